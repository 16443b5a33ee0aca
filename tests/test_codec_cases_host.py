"""CPU-only: what keeps tests/test_gpu_byword_codec.py from being vacuous, asserted on the C oracle alone.  The case table of
tests/codec_cases.py reaches every outcome of the Reed-Solomon decoder often enough (FLOORS, per nsym), puts an error on every special
byte position, and arrives at the step kernels' codec as chosen: the Viterbi detector returns a noiseless word exactly, and the
trained ViterbiNet of G7 at 40 dB nearly so.  reference_step is tied to the reference's own numbers through golden G9."""
import numpy as np
import pytest

import codec_cases as C


def _totals(nsym, detected):
    tot = {}
    for n in C.lengths(nsym):
        for key, v in C.outcome_counts(detected(nsym, n), C.batch(nsym, n)).items():
            tot[key] = tot.get(key, 0) + v
    return tot


def _assert_floors(nsym, tot, what):
    print(f"{what} nsym={nsym}: {tot}")
    assert tot["clean"] >= C.FLOORS["clean"], (what, nsym, tot)
    if nsym >= 2:
        assert tot["corrected"] >= C.FLOORS["corrected"], (what, nsym, tot)
    if nsym % 2:
        assert tot["status1"] >= C.FLOORS["status1"], (what, nsym, tot)
    else:
        assert tot["wrong0"] >= C.FLOORS["wrong0"], (what, nsym, tot)
    assert tot["failed_within_t"] == 0, (what, nsym, tot)  # no word with e <= t errors is decoded wrongly
    assert tot["status2"] == 0, (what, nsym, tot)


@pytest.mark.parametrize("nsym", C.NSYMS)
def test_table_reaches_every_decoder_outcome(oracle, nsym):
    """The table as built (= as the Viterbi step detects it): per nsym at least 30 clean words, 40 corrected ones (nsym >= 2), 40 'too
    many errors' (odd nsym) or 40 wrong messages with status 0 (even nsym); nothing within the capacity fails, status 2 nowhere."""
    _assert_floors(nsym, _totals(nsym, lambda s, n: C.batch(s, n)["word"]), "VA table")


@pytest.mark.parametrize("nsym,n", C.CASES)
def test_table_puts_errors_where_it_says(oracle, nsym, n):
    b = C.batch(nsym, n)
    k, t = n - nsym, nsym // 2
    R = len(b["pos"])
    assert b["msg"].shape == (R, 8 * k) and b["word"].shape == (R, 8 * n) and 8 * n <= 1024 and k >= 1
    assert np.array_equal(b["cw"], oracle.rs_encode_bits(b["msg"], nsym)) and np.all(b["msg"][:, 0] == 0) and np.all(b["word"][:, 0] == 0)
    diff = C.pack(b["word"]) != C.pack(b["cw"])
    for r, pos in enumerate(b["pos"]):  # the corrupted bytes are exactly the listed ones (every error value is non-zero)
        assert len(set(pos)) == len(pos) and sorted(pos) == np.flatnonzero(diff[r]).tolist(), (r, pos)
    counts = [len(p) for p, po in zip(b["pos"], b["parity_only"]) if not po]
    for e in range(min(n, t + 2) + 1):
        assert counts.count(e) >= 6, e
    assert max(counts) == min(n, t + 2)
    po = [p for p, f in zip(b["pos"], b["parity_only"]) if f]
    assert sorted(len(p) for p in po) == list(range(1, min(nsym, t + 2) + 1)) and all(min(p) >= k for p in po)
    hit = {p for pos in b["pos"] for p in pos}
    spec = C.special_positions(nsym, n)
    assert set(spec) == {p for p in (0, k - 1, k, n - 1, 63, 64, n // 2) if 0 <= p < n}
    assert set(spec) <= hit, sorted(set(spec) - hit)
    if n >= 65:
        assert any(63 in pos and 64 in pos for pos in b["pos"])
        if t >= 2:  # ... and one of them within the capacity: corrected across the seam
            assert any(63 in pos and 64 in pos and len(pos) <= t for pos in b["pos"])


@pytest.mark.parametrize("nsym", C.NSYMS)
def test_viterbi_returns_the_noiseless_word(oracle, nsym):
    """Precondition of the VA GPU test: va_decode(clean_channel(word, 0)) is the word, bit for bit, for the whole table."""
    pri = C.channel()[1]
    for n in C.lengths(nsym):
        word = C.batch(nsym, n)["word"]
        dec = oracle.va_decode(C.clean_channel(word, 0), pri, want_final=False)
        assert np.array_equal(dec, word), (nsym, n, np.argwhere(dec != word)[:4].tolist())


@pytest.mark.parametrize("nsym", C.NSYMS)
def test_viterbinet_table_keeps_the_floors(oracle, golden, nsym):
    """Precondition of the ViterbiNet GPU test: G7's network at 40 dB flips a few bits per batch; the floors hold on what it detects."""
    w = C.g7_weights(golden)
    stray = []

    def detected(s, n):
        dec = oracle.vnet_decode(C.vnet_rx(s, n), w)
        stray.append(int((dec != C.batch(s, n)["word"]).sum()))
        return dec

    tot = _totals(nsym, detected)
    print(f"stray bits per batch: {stray}")
    _assert_floors(nsym, tot, "ViterbiNet table")


def test_clean_channel_is_the_transmit_kernels_sum():
    """clean_channel against the defining sum written out element by element, and its noise against the seed."""
    h = C.channel()[0][0]
    rng = np.random.RandomState(5)
    c = rng.randint(0, 2, (3, 24)).astype(np.float32)
    want = np.zeros((3, 24))
    for b in range(3):
        for t in range(24):
            want[b, t] = sum(h[C.L - 1 - i] * (1.0 - 2.0 * (c[b, t + i] if t + i < 24 else 0.0)) for i in range(C.L))
    assert np.array_equal(C.clean_channel(c, 0), want.astype(np.float32))
    noisy = C.clean_channel(c, 0.5, seed=9)
    assert np.array_equal(noisy, (want + 0.5 * np.random.RandomState(9).standard_normal((3, 24))).astype(np.float32))


@pytest.mark.parametrize("coef", ["time_decay", "cost2100"])
def test_reference_step_reproduces_g9(oracle, golden, coef):
    """reference_step on G9's recorded detected words gives the reference's recorded ser_by_word on the data blocks (trainer.py:301,309),
    and a label word that is the detection exactly where the block has errors (:322-323)."""
    g = golden("g9_by_word_va")
    nsym = int(g[f"{coef}_meta"][7])
    det, tx = g[f"{coef}_detected"].astype(np.float32), g[f"{coef}_tx"].astype(np.float32)
    data, ref = g[f"{coef}_data_indices"], g[f"{coef}_ser_by_word"]
    K = tx.shape[1]
    out = C.reference_step(det[data], tx[data], nsym, False)
    assert np.array_equal(np.rint(ref[data] * K).astype(np.int64), out["nerr"])
    assert np.allclose(out["nerr"] / K, ref[data], rtol=1e-6, atol=1e-7)  # (the reference's mean is float32)
    assert np.count_nonzero(out["nerr"]) > 0 and np.count_nonzero(out["nerr"] == 0) > 0
    bad = out["nerr"] > 0
    assert np.array_equal(out["label_word"][bad], det[data][bad]) and np.array_equal(out["label_word"][~bad], out["enc"][~bad])
    assert np.array_equal(out["enc"], oracle.rs_encode_bits(out["msg"], nsym))
    pilots = np.setdiff1d(np.arange(tx.shape[0]), data)
    pil = C.reference_step(None, tx[pilots], nsym, True)
    assert pil["msg"] is None and not pil["nerr"].any() and np.array_equal(pil["enc"], pil["label_word"])
    assert np.array_equal(pil["enc"][:, :K], tx[pilots])  # systematic
    assert np.array_equal(pil["labels"].reshape(-1), oracle.calculate_states(C.L, pil["enc"]))
