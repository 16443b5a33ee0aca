"""CPU-only: the NumPy restatement of the word generator (word_gen_ref.py) checked on its own, before tests/test_gpu_word_gen.py holds
the kernels to it -- Philox against the Random123 known answers, the uniform mapping on the 32-bit words where float32 rounding
decides, the samples' distribution, and the ISI sum against an independently written formula.

The last test shows that the comparisons of test_gpu_word_gen.py flag a wrong generator, without running one: each mutation is applied
to the restatement and compared, by the same rule, with the unmutated data."""
import numpy as np
import pytest

import word_gen_ref as R


def test_philox_known_answers():
    kat = R.philox4x32_10(np.array([[0, 0, 0, 0]], np.uint32), (0, 0))
    assert kat[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert R.philox4x32_10(np.array([[0xFFFFFFFF] * 4], np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0].tolist() == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert R.philox4x32_10(np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32), (0xA4093822, 0x299F31D0))[0].tolist() == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_uniform_mapping_edges():
    """The true ranges of the two uniforms (csrc/word_gen.inc's header): u1 in [2^-32, 1], u2 in [0, 1], |z| <= sqrt(64 ln 2)."""
    u1 = lambda a: float(R.u1_ref(np.uint32(a)))  # noqa: E731
    u2 = lambda b: float(R.u2_ref(np.uint32(b)))  # noqa: E731
    assert u1(0) == u1(1) == 2.0 ** -32
    assert u1(0xFFFFFFFF) == 1.0
    assert u1(0xFFFFFF7F) == 1.0 - 2.0 ** -24
    assert u2(0) == 0.0
    assert u2(0xFFFFFFFF) == u2(0xFFFFFF80) == 1.0
    assert u2(0xFFFFFF7F) == 1.0 - 2.0 ** -24
    assert R.u1_ref(np.uint32(5)).dtype == np.float32 and R.u2_ref(np.uint32(5)).dtype == np.float32
    z0, z1, r = R.box_muller_ref(np.array([0, 1, 0xFFFFFFFF], np.uint32), np.array([0, 0x40000000, 0x80000000], np.uint32))
    assert r[0] == r[1] == R.R_MAX and abs(R.R_MAX - 6.6604) < 1e-4
    assert z0[0] == R.R_MAX and z1[0] == 0.0  # angle 0
    assert abs(z0[1]) < 1e-15 and z1[1] == R.R_MAX  # a quarter revolution
    assert r[2] == 0.0 and z0[2] == 0.0 and z1[2] == 0.0  # u1 rounded to 1: the sample is 0
    a = np.random.RandomState(1).randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    assert R.u1_ref(a).min() >= 2.0 ** -32 and R.u1_ref(a).max() <= 1.0 and R.u2_ref(a).min() >= 0.0 and R.u2_ref(a).max() <= 1.0


MOMENT_CASES = ((3450002, 512, 1000), (0x0123456789ABCDEF, 300, 257), (7, 64, 129))


@pytest.mark.parametrize("seed,B,T", MOMENT_CASES)
def test_restated_noise_is_standard_normal(seed, B, T):
    """The 5 sigma limits of test_word_generator_bits_are_philox_and_noise_is_standard_normal, on the restatement alone."""
    import scipy.stats

    z, r = R.noise_ref(seed, B, T)
    bits = R.bits_ref(seed, B, T).astype(np.float64)
    n = z.size
    assert z.shape == r.shape == bits.shape == (B, T)
    assert np.all(np.abs(z) <= r) and r.max() <= R.R_MAX
    stats = {"mean": z.mean() * np.sqrt(n), "var": (z.var() - 1) / np.sqrt(2 / n), "kurtosis": scipy.stats.kurtosis(z.ravel()) / np.sqrt(24 / n),
             "skew": scipy.stats.skew(z.ravel()) / np.sqrt(6 / n), "lag1": np.mean(z[:, :-1] * z[:, 1:]) * np.sqrt(n),
             "bits": np.mean(z * (1 - 2 * bits)) * np.sqrt(n), "bit mean": (bits.mean() - 0.5) / (0.5 / np.sqrt(n)),
             "bit lag1": np.mean((1 - 2 * bits[:, :-1]) * (1 - 2 * bits[:, 1:])) * np.sqrt(n)}
    p = scipy.stats.kstest(z.ravel()[:200000], "norm").pvalue
    print(f"seed {seed:#x} B {B} T {T}: " + " ".join(f"{k} {v:+.2f} sigma" for k, v in stats.items()) + f" KS p {p:.3f}")
    for k, v in stats.items():
        assert abs(v) < 5, (k, v)
    assert p > 1e-3


def test_words_are_addressed_globally():
    """word0 shifts the word index, across 2^32 as well: rows of a call are the rows of any call that contains them."""
    seed, T = 0x0123456789ABCDEF, 130
    w0 = 2 ** 32 - 3
    z, r = R.noise_ref(seed, 8, T, word0=w0)
    for i in (0, 2, 3, 7):
        zi, ri = R.noise_ref(seed, 1, T, word0=w0 + i)
        assert np.array_equal(zi[0], z[i]) and np.array_equal(ri[0], r[i])
        assert np.array_equal(R.bits_ref(seed, 1, T, word0=w0 + i)[0], R.bits_ref(seed, 8, T, word0=w0)[i])
    assert not np.array_equal(R.noise_ref(seed, 1, T, word0=2 ** 32)[0], R.noise_ref(seed, 1, T, word0=0)[0])  # b_hi counts
    assert not np.array_equal(R.bits_ref(seed, 1, T, word0=2 ** 32), R.bits_ref(seed, 1, T, word0=0))
    assert np.array_equal(R.bits_ref(seed, 3, T)[:, :77], R.bits_ref(seed, 3, 77))  # and a shorter word is a prefix


def _isi_direct(bits, h, L):
    """The channel as its formula is written: the [L, T] matrix of the shifted symbols s = 1 - 2 c, padded with +1, times the reversed
    taps of the word's row."""
    B, T = bits.shape
    s = np.concatenate([1.0 - 2.0 * bits.astype(np.float64), np.ones((B, L))], axis=1)
    out = np.empty((B, T))
    for b in range(B):
        shifted = np.stack([s[b, i:i + T] for i in range(L)])  # [L, T]
        out[b] = h[b % h.shape[0], ::-1] @ shifted
    return out


@pytest.mark.parametrize("Bh", (1, 3))
@pytest.mark.parametrize("L", (1, 2, 4, 8, 16))
def test_isi_ref_against_the_direct_formula(L, Bh):
    rng = np.random.RandomState(100 * L + Bh)
    h = rng.normal(0, 1, (Bh, L))
    for T in (1, 3, L, 131):
        bits = R.bits_ref(5, 7, T)
        got, want = R.isi_ref(bits, h, L), _isi_direct(bits, h, L)
        assert got.shape == (7, T) and got.dtype == np.float64
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(h).sum(axis=1)[np.arange(7) % Bh, None]), (L, Bh, T)
    assert np.array_equal(R.isi_ref(np.zeros((2, 5), np.uint8), h, L), np.repeat(_seq_sum(h[np.arange(2) % Bh]), 5, axis=1))


def _seq_sum(hb):
    acc = np.zeros(hb.shape[0])
    for k in range(hb.shape[1]):
        acc = acc + hb[:, hb.shape[1] - 1 - k]
    return acc[:, None]


def test_isi_ref_exact_zero_on_opposite_taps():
    """h = [1, 1] at L = 2: the sum is exactly 0 wherever the two bits differ, and +0.0 (the kernels add to +0.0 in this order)."""
    bits = R.bits_ref(11, 3, 64)
    y = R.isi_ref(bits, np.array([[1.0, 1.0]]), 2)
    nxt = np.concatenate([bits[:, 1:], np.zeros((3, 1), np.uint8)], axis=1)
    assert np.array_equal(y == 0.0, bits != nxt) and 0.3 < np.mean(y == 0.0) < 0.7
    assert not np.any(np.signbit(y[y == 0.0]))
    assert set(np.unique(y)) == {-2.0, 0.0, 2.0}


def test_fused_route_case_has_no_decision_on_a_knife_edge(oracle, golden):
    """test_gpu_word_gen.py (e) compares integers, which is exact only if no decision of its 320 symbols flips within the noise
    tolerance.  On the CPU oracle's ViterbiNet the first seed has none even at TAU_MAX, the widest tolerance the GPU test may use."""
    g7 = golden("g7_by_word")
    w = [g7[f"w{k}"] for k in range(6)]
    bits, y, y_lo, y_hi = R.mc_case(R.MC_SEEDS[0], tau=R.TAU_MAX)
    assert bits.shape == y.shape == (R.MC_WORDS, R.MC_T) and np.all(y_lo <= y) and np.all(y <= y_hi) and np.any(y_lo < y_hi)
    edge = R.knife_edge_symbols(lambda a: oracle.vnet_decode(a, w), y, y_lo, y_hi)
    errors = int(np.count_nonzero(oracle.vnet_decode(y, w) != bits))
    print(f"seed {R.MC_SEEDS[0]}: {edge} decisions on a knife edge at tau = 2^-10, {errors} bit errors of {bits.size}")
    assert edge == 0
    assert R.knife_edge_symbols(lambda a: oracle.vnet_decode(a, w), y, y - np.float32(0.5), y + np.float32(0.5)) > 0  # the count counts
    assert R.TAU <= R.TAU_MAX == 2.0 ** -10


# ------------------------------------------------------------ the GPU comparisons would flag a wrong generator
TAU = 2.0 ** -10  # the largest tolerance test_gpu_word_gen.py may use (its condition on tau)


def _noise_mismatches(z, z_ref, r_ref, tau=TAU):
    """test_gpu_word_gen.py's rule (b): the number of samples with |z - z_ref| > tau r_ref + 2^-149."""
    return int(np.count_nonzero(np.abs(z - z_ref) > tau * r_ref + 2.0 ** -149))


def test_the_comparisons_flag_wrong_generators(monkeypatch):
    seed, B, T, L = 0x0123456789ABCDEF, 37, 1000, 4
    z_ref, r_ref = R.noise_ref(seed, B, T)
    assert _noise_mismatches(z_ref, z_ref, r_ref) == 0
    assert _noise_mismatches(z_ref.astype(np.float32).astype(np.float64), z_ref, r_ref, 2.0 ** -22) == 0  # float32 storage passes

    # sin and cos swapped: samples 4q and 4q + 1 trade places
    swapped = z_ref.reshape(B, T // 2, 2)[:, :, ::-1].reshape(B, T)
    bad = _noise_mismatches(swapped, z_ref, r_ref)
    print(f"sin <-> cos: {bad} of {B * T} samples outside tau r")
    assert bad > 0.9 * B * T

    # the noise counter's last word 0: the noise is made from the words of the bit stream
    real_words = R._words
    monkeypatch.setattr(R, "_words", lambda seed, B, n, word0, stream: real_words(seed, B, n, word0, 0))
    z_bad, _ = R.noise_ref(seed, B, T)
    monkeypatch.setattr(R, "_words", real_words)
    bad = _noise_mismatches(z_bad, z_ref, r_ref)
    print(f"counter (q, b_lo, b_hi, 0): {bad} of {B * T} samples outside tau r")
    assert bad > 0.9 * B * T

    # radians for revolutions, and a noise amplitude off by 2^-9 (twice tau)
    u2 = R.u2_ref(real_words(seed, B, T // 4, 0, 1)[:, :, 1]).astype(np.float64)  # of samples 4q
    assert _noise_mismatches(r_ref[:, ::4] * np.cos(u2), z_ref[:, ::4], r_ref[:, ::4]) > 0.9 * B * T / 4
    assert _noise_mismatches(z_ref * (1 + 2.0 ** -9), z_ref, r_ref) > 0.5 * B * T

    # `next` forced to 0: the look-ahead past a 128-bit group reads zeros -- rule (a), exact equality of the ISI sum
    h = np.exp(-0.2 * np.arange(L)).reshape(1, L)
    bits = R.bits_ref(seed, B, T)
    y = R.isi_ref(bits, h, L).astype(np.float32)
    look = np.concatenate([bits, np.zeros((B, L), np.uint8)], axis=1)
    acc = np.zeros((B, T))
    for k in range(L):
        t = np.arange(T)
        crosses = ((t // 4 * 4) % 128 == 124) & (t + k >= (t // 128 + 1) * 128)  # the last quad of a group looking into the next
        c = np.where(crosses[None, :], 0, look[:, k:k + T])
        acc = acc + np.where(c != 0, -h[0, L - 1 - k], h[0, L - 1 - k])
    wrong = np.argwhere(acc.astype(np.float32) != y)
    print(f"next = 0: {len(wrong)} of {B * T} samples differ, all at t % 128 in {sorted(set((wrong[:, 1] % 128).tolist()))}")
    assert len(wrong) > 0 and set((wrong[:, 1] % 128).tolist()) <= {125, 126, 127}
