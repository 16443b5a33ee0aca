"""GPU tests (pytest -m gpu) of the codec inside the by-word step kernels (byword_step.inc: lane-per-byte syndromes, two-ballot root
search, one-lane Berlekamp-Massey and Forney, closed-form or divided parity, popcount error count, label word and trellis states) and
of the stand-alone codec (rs_codec.inc), on the chosen error patterns of tests/codec_cases.py.  The expected values come from the C
oracle alone (codec_cases.reference_step; no mvn.rs_* call); tests/test_codec_cases_host.py shows on the CPU that the table reaches
every decoder outcome and arrives at the codec as chosen.  Every comparison is exact; one launch per (nsym, n) batch."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as C
import meta_viterbinet_amd as mvn
from meta_viterbinet_amd.trials import TrialBank
from step_call import SENTINEL, padded as _padded, step

pytestmark = pytest.mark.gpu

ALL = ("dec", "msg", "enc", "lw", "labels", "nerr")
LD_SHAPES = [(2, 17), (8, 65), (5, 128)]
REQUESTS = [("nerr",), ("nerr", "labels"), ("msg", "nerr"), ("enc",), ("lw", "labels")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g7w(golden, dev):
    w = C.g7_weights(golden)
    return w, [torch.as_tensor(a).to(dev).contiguous() for a in w]


def _explain(b, name, got, want, dec=None):
    """nsym, n, the word's chosen error positions and the first differing element of output `name`."""
    idx = np.argwhere(np.asarray(got) != np.asarray(want))
    r = int(idx[0][0])
    extra = "" if dec is None else f", bytes that differ from the codeword after detection {np.flatnonzero(C.pack(dec)[r] != C.pack(b['cw'])[r]).tolist()}"
    return (f"nsym={b['nsym']} n={b['n']} word {r} (errors at bytes {b['pos'][r]}{extra}): {name}{idx[0].tolist()} = "
            f"{np.asarray(got)[tuple(idx[0])]}, expected {np.asarray(want)[tuple(idx[0])]}; {len(idx)} elements differ")


def _assert_step(b, out, row, ref, dec=None, names=("msg", "nerr", "enc", "lw", "labels")):
    """The requested outputs' rows equal the reference step's, and every padding element kept its sentinel."""
    expect = {"dec": dec, "msg": ref["msg"], "nerr": ref["nerr"], "enc": ref["enc"], "lw": ref["label_word"], "labels": ref["labels"]}
    for name in names:
        if name not in out:
            continue
        got = out[name] if name == "nerr" else out[name][:, :row[name]]
        if not np.array_equal(got, expect[name]):
            pytest.fail(_explain(b, name, got, expect[name], dec))
        if name != "nerr":
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"nsym={b['nsym']} n={b['n']}: padding of {name} written"


def _priors(dev, Bp=1):
    return torch.as_tensor(np.repeat(C.channel()[1], Bp, axis=0)).to(dev).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the whole table
@pytest.mark.parametrize("nsym,n", C.CASES)
def test_va_step_on_chosen_error_patterns(oracle, dev, nsym, n):
    """mvn_va_byword_step_f32 on the noiseless words: dec IS the chosen word, and everything after it equals the oracle's step.  Once
    with one row of priors for all words, once with a row per word (all equal)."""
    b = C.batch(nsym, n)
    R = b["word"].shape[0]
    rx = C.clean_channel(b["word"], 0)
    ref = C.reference_step(b["word"], b["msg"], nsym, False)
    for Bp in (1, R):
        out, row = step(dev, "running", "va", rx, b["msg"], nsym, False, pri=_priors(dev, Bp), Bp=Bp)
        if not np.array_equal(out["dec"], b["word"]):  # the precondition: the codec saw the chosen pattern
            pytest.fail("detection: " + _explain(b, "dec", out["dec"], b["word"]))
        _assert_step(b, out, row, ref, b["word"])


@pytest.mark.parametrize("nsym,n", C.CASES)
def test_vnet_step_on_chosen_error_patterns(oracle, dev, g7w, nsym, n):
    """mvn_vnet_byword_step_f32 with G7's weights (one set for all words: w_stride NULL) on the words at 40 dB: dec is the oracle's
    detection, everything after it the oracle's step on that detection."""
    b = C.batch(nsym, n)
    rx = C.vnet_rx(nsym, n)
    dec = oracle.vnet_decode(rx, g7w[0])
    ref = C.reference_step(dec, b["msg"], nsym, False)
    out, row = step(dev, "running", "vnet", rx, b["msg"], nsym, False, weights=[mvn._lib.ptr(t) for t in g7w[1]])
    if not np.array_equal(out["dec"], dec):
        pytest.fail("detection: " + _explain(b, "dec", out["dec"], dec, dec))
    _assert_step(b, out, row, ref, dec)


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("nsym", C.NSYMS)
def test_vnet_step_with_a_weight_set_per_word(oracle, golden, dev, nsym, n):
    """R weight sets through w_stride (a TrialBank's rows, trial r = G7's weights times its own factor): word r is detected with set r,
    and its codec outputs follow from ITS detection."""
    b = C.batch(nsym, n)
    R = b["word"].shape[0]
    rx = C.vnet_rx(nsym, n)
    base = C.g7_weights(golden)
    w = [[(a * np.float32(f)).astype(np.float32) for a in base] for f in np.linspace(0.97, 1.03, R)]
    bank = TrialBank(w, 16, C.L, dev)
    dec = np.concatenate([oracle.vnet_decode(rx[r:r + 1], w[r]) for r in range(R)])
    ref = C.reference_step(dec, b["msg"], nsym, False)
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = step(dev, "running", "vnet", rx, b["msg"], nsym, False, weights=wp, w_stride=[bank.P] * 6)
    if not np.array_equal(out["dec"], dec):
        pytest.fail("detection: " + _explain(b, "dec", out["dec"], dec, dec))
    _assert_step(b, out, row, ref, dec)


@pytest.mark.parametrize("kind", ["va", "vnet"])
@pytest.mark.parametrize("nsym,n", C.CASES)
def test_pilot_step_encodes_the_transmitted_word(oracle, dev, g7w, kind, nsym, n):
    """Pilot step: enc = label word = encode(tx) by the oracle, labels its trellis states, nerr 0; dec and msg keep their sentinel."""
    b = C.batch(nsym, n)
    kw = dict(pri=_priors(dev)) if kind == "va" else dict(weights=[mvn._lib.ptr(t) for t in g7w[1]])
    out, row = step(dev, "running", kind, C.clean_channel(b["word"], 0), b["msg"], nsym, True, **kw)
    ref = C.reference_step(None, b["msg"], nsym, True)
    assert np.array_equal(ref["enc"], oracle.rs_encode_bits(b["msg"], nsym)) and not ref["nerr"].any()
    _assert_step(b, out, row, ref, names=("nerr", "enc", "lw", "labels"))
    assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])


@pytest.mark.parametrize("variant", ["running", "path", "list"])
@pytest.mark.parametrize("kind", ["va", "vnet"])
@pytest.mark.parametrize("T,nsym", [(16, 1), (40, 3)], ids=["closed_form", "generator"])
def test_pilot_step_needs_no_received_word(oracle, dev, g7w, kind, variant, T, nsym):
    """A pilot through every entry point with rx NULL (and, for VA, the priors NULL), R = 2, list_bytes = nsym: enc = label word = the
    oracle's rs_encode of tx, labels = calculate_states of that word, nerr 0; dec, msg, delta and choice keep their sentinel."""
    tx = np.random.RandomState(100 * T + nsym).randint(0, 2, (2, T - 8 * nsym)).astype(np.float32)
    kw = dict(pri=None) if kind == "va" else dict(weights=g7w[1])
    out, row = step(dev, variant, kind, None, tx, nsym, True, m=nsym, **kw)
    word = oracle.rs_encode_bits(tx, nsym)
    assert np.array_equal(out["enc"], word) and np.array_equal(out["lw"], word)
    assert np.array_equal(out["labels"], oracle.calculate_states(C.L, word).reshape(2, T))
    assert not out["nerr"].any()
    for name in set(out) - {"enc", "lw", "labels", "nerr"}:
        assert np.all(out[name] == SENTINEL[name]), name
    assert {"dec", "msg"} <= set(out) and (variant != "list" or {"delta", "choice"} <= set(out))


# ------------------------------------------------------------------------------------------- leading dimensions, optional outputs
def _kind_inputs(oracle, dev, g7w, kind, nsym, n):
    b = C.batch(nsym, n)
    if kind == "va":
        return b, C.clean_channel(b["word"], 0), b["word"], dict(pri=_priors(dev))
    rx = C.vnet_rx(nsym, n)
    return b, rx, oracle.vnet_decode(rx, g7w[0]), dict(weights=[mvn._lib.ptr(t) for t in g7w[1]])


@pytest.mark.parametrize("pilot", [False, True])
@pytest.mark.parametrize("kind", ["va", "vnet"])
@pytest.mark.parametrize("nsym,n", LD_SHAPES)
def test_step_honours_every_leading_dimension(oracle, dev, g7w, kind, nsym, n, pilot):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's: the outputs equal the compact
    run's (and the oracle's step), and no padding element of any output is written."""
    b, rx, dec, kw = _kind_inputs(oracle, dev, g7w, kind, nsym, n)
    T, K = 8 * n, 8 * (n - nsym)
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6}
    compact, row = step(dev, "running", kind, rx, b["msg"], nsym, pilot, **kw)
    wide, _ = step(dev, "running", kind, rx, b["msg"], nsym, pilot, ld=ld, **kw)
    for name in ALL:
        got = wide[name] if name == "nerr" else wide[name][:, :row[name]]
        if not np.array_equal(got, compact[name]):
            pytest.fail("against the compact run: " + _explain(b, name, got, compact[name], dec))
        if name != "nerr":
            assert np.all(wide[name][:, row[name]:] == SENTINEL[name]), f"padding of {name} written"
    ref = C.reference_step(dec, b["msg"], nsym, pilot)
    if pilot:
        assert np.all(wide["dec"] == SENTINEL["dec"]) and np.all(wide["msg"] == SENTINEL["msg"])
        _assert_step(b, wide, row, ref, names=("nerr", "enc", "lw", "labels"))
    else:
        _assert_step(b, wide, row, ref, dec, names=ALL)


@pytest.mark.parametrize("want", REQUESTS, ids=["+".join(r) for r in REQUESTS])
@pytest.mark.parametrize("kind", ["va", "vnet"])
@pytest.mark.parametrize("nsym,n", LD_SHAPES)
def test_step_with_some_outputs_only(oracle, dev, g7w, kind, nsym, n, want):
    """Outputs not requested are NULL; what is requested equals the all-outputs run (and the oracle's step)."""
    b, rx, dec, kw = _kind_inputs(oracle, dev, g7w, kind, nsym, n)
    full, row = step(dev, "running", kind, rx, b["msg"], nsym, False, **kw)
    part, _ = step(dev, "running", kind, rx, b["msg"], nsym, False, want=want, **kw)
    assert sorted(part) == sorted(want)
    for name in want:
        if not np.array_equal(part[name], full[name]):
            pytest.fail("against the all-outputs run: " + _explain(b, name, part[name], full[name], dec))
    _assert_step(b, part, row, C.reference_step(dec, b["msg"], nsym, False), dec, names=want)


# ------------------------------------------------------------------------------------------------------- the stand-alone codec
def _rs_call(dev, fn, x, ld_in, width_out, ld_out, nbits, nsym, with_status):
    B = x.shape[0]
    x_d = _padded(x, ld_in, np.nan, dev)
    out = torch.full((B, ld_out), 7.0, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev) if with_status else None
    lib = mvn._lib.load()
    if with_status:
        rc = lib.mvn_rs_decode_bits_f32(mvn._lib.ptr(x_d), ld_in, mvn._lib.ptr(out), ld_out, mvn._lib.ptr(status), B, nbits, nsym,
                                        mvn._lib.current_stream(dev))
    else:
        rc = lib.mvn_rs_encode_bits_f32(mvn._lib.ptr(x_d), ld_in, mvn._lib.ptr(out), ld_out, B, nbits, nsym, mvn._lib.current_stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    out = out.cpu().numpy()
    assert np.all(out[:, width_out:] == 7.0), f"{fn}: padding written"
    return out[:, :width_out], None if status is None else status.cpu().numpy()


@pytest.mark.parametrize("nsym,n", C.CASES)
def test_standalone_codec_on_chosen_error_patterns(oracle, dev, nsym, n):
    """mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32 through the raw ABI on the same table, the batch repeated to B = 129 (a full
    128-word workgroup and one word more) and one word alone, with ld_in = 8n + 3 and ld_out = 8k + 5 (decode; the other way round for
    encode): message and status, and the codeword, equal the oracle's; the padding is untouched."""
    b = C.batch(nsym, n)
    k, R = n - nsym, b["word"].shape[0]
    rows = np.arange(129) % R
    lone = next(r for r, pos in enumerate(b["pos"]) if len(pos) == max(1, nsym // 2))  # (corrected where the code corrects at all)
    for sel in (rows, np.array([lone])):
        word, tx = b["word"][sel], b["msg"][sel]
        want_msg, want_st = oracle.rs_decode_bits(word, nsym, want_status=True)
        msg, st = _rs_call(dev, "decode", word, 8 * n + 3, 8 * k, 8 * k + 5, 8 * n, nsym, True)
        sub = dict(b, pos=[b["pos"][r] for r in sel])
        if not np.array_equal(st, want_st):
            pytest.fail(f"B={len(sel)} " + _explain(sub, "status", st, want_st))
        if not np.array_equal(msg, want_msg):
            pytest.fail(f"B={len(sel)} " + _explain(sub, "msg", msg, want_msg))
        cw, _ = _rs_call(dev, "encode", tx, 8 * k + 5, 8 * n, 8 * n + 3, 8 * k, nsym, False)
        want_cw = oracle.rs_encode_bits(tx, nsym)
        if not np.array_equal(cw, want_cw):
            pytest.fail(f"B={len(sel)} " + _explain(sub, "codeword", cw, want_cw))
