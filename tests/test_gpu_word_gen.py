"""mvn_generate_words_f32 (csrc/word_gen.inc: generate_quad, the one generator of every Monte-Carlo route) held to the NumPy restatement
of tests/word_gen_ref.py, sample for sample.  What can be exact is asserted exactly, the one thing that cannot gets the one tolerance:

  (a) sigma = 0: the transmitted bits and the float64 ISI sum, bit for bit, at every L and at the word lengths that put the last quad
      and the look-ahead across a 128-bit group boundary in every position; mvn.transmit (isi_awgn_kernel) gives the same array
  (b) zero taps, sigma = 1: y is the device's float32 Box-Muller sample itself, within R.TAU r_ref of the float64 restatement
  (c) y = float32(isi_ref + sigma float64(z of (b))) bit for bit for general taps, L and sigma: the noise is a pure function of
      (seed, word, position), and the composition adds nothing of its own
  (d) the C entry point's call shapes: NULL tx, leading dimensions, prefixes, empty calls
  (e) mvn.vnet_monte_carlo across word index 2^32 counts what the restatement's words give

tests/test_word_gen_ref_host.py checks the restatement itself and shows that these comparisons flag wrong generators."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import word_gen_ref as R

pytestmark = pytest.mark.gpu

SEEDS = (3450002, 0x0123456789ABCDEF)  # the second has a non-zero high half
SHAPES = ((300, 257), (37, 1000), (5, 1))
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def bits_of(a):
    """float32 array -> its bit patterns (a comparison that tells -0.0 from +0.0)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def generate(dev, seed, B, T, h, sigma, L, want_tx=True, y_ld=None, tx_ld=None, rows=None, expect=0):
    """One call of the C entry point.  Returns (tx, y) as host arrays INCLUDING their padding, [rows or B, ld], pre-filled with
    SENTINEL (tx None when not asked for)."""
    y_ld = T if y_ld is None else y_ld
    tx_ld = T if tx_ld is None else tx_ld
    n = B if rows is None else rows
    hd = torch.as_tensor(np.ascontiguousarray(h, np.float64).reshape(-1, L), device=dev)
    y = torch.full((n, max(y_ld, 1)), SENTINEL, dtype=torch.float32, device=dev)
    tx = torch.full((n, max(tx_ld, 1)), SENTINEL, dtype=torch.float32, device=dev) if want_tx else None
    rc = mvn._lib.load().mvn_generate_words_f32(mvn._lib.ptr(tx), tx_ld, mvn._lib.ptr(y), y_ld, mvn._lib.ptr(hd), hd.shape[0], float(sigma),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, B, T, L, mvn._lib.current_stream(dev))
    assert rc == expect, rc
    torch.cuda.synchronize(dev)
    return (None if tx is None else tx.cpu().numpy()), y.cpu().numpy()


@pytest.fixture(scope="module")
def refs():
    """(seed, B, T) -> (bits_ref, z_ref, r_ref): computed once, shared, never written to."""
    made = {}

    def get(seed, B, T):
        if (seed, B, T) not in made:
            made[(seed, B, T)] = (R.bits_ref(seed, B, T),) + R.noise_ref(seed, B, T)
            for a in made[(seed, B, T)]:
                a.setflags(write=False)
        return made[(seed, B, T)]

    return get


@pytest.fixture(scope="module")
def z_kernel(dev):
    """(seed, B, T) -> the device's noise samples: zero taps and snr = 0 through the wrapper (sigma exactly 1.0), so that
    y = float32(0.0 + 1.0 * double(z)) is z with no further rounding."""
    made = {}

    def get(seed, B, T):
        if (seed, B, T) not in made:
            assert R.sigma_of(0.0) == 1.0
            made[(seed, B, T)] = mvn.generate_words(B, T, np.zeros((1, 4)), 0.0, 4, dev, seed)[1].cpu().numpy()
            made[(seed, B, T)].setflags(write=False)
        return made[(seed, B, T)]

    return get


# ---------------------------------------------------------------- (a) bits and ISI sum, exact
TS_A = (1, 2, 3, 4, 5, 31, 32, 33, 124, 125, 127, 128, 129, 131, 255, 256, 257, 260, 385)
BS_A = (1, 3, 67)


def taps_a(L, Bh, kind):
    if kind == "ones":
        return np.ones((Bh, L))
    return np.random.RandomState(1000 * L + Bh).normal(0, 1, (Bh, L))


@pytest.mark.parametrize("L,kind", [(L, "random") for L in (1, 2, 3, 4, 5, 8, 15, 16)] + [(2, "ones")])
def test_bits_and_isi_sum_are_exact(dev, L, kind):
    seed = SEEDS[1] + L
    checked = zeros = 0
    for T in TS_A:
        for B in BS_A:
            bits = R.bits_ref(seed, B, T)
            for Bh in sorted({1, 3, B}):
                h = taps_a(L, Bh, kind)
                want = R.isi_ref(bits, h, L).astype(np.float32)
                tx, y = generate(dev, seed, B, T, h, 0.0, L)
                tag = f"L {L} T {T} B {B} Bh {Bh}"
                assert np.array_equal(tx, bits.astype(np.float32)), tag
                bad = np.argwhere(bits_of(y) != bits_of(want))
                assert len(bad) == 0, f"{tag}: {len(bad)} samples differ, first (b, t) = {bad[0].tolist()}: {y[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
                clean = mvn.transmit(torch.as_tensor(tx, device=dev), h, 9.0, L, None).cpu().numpy()
                assert np.array_equal(bits_of(clean), bits_of(want)), f"{tag}: mvn.transmit"
                checked += want.size
                zeros += int(np.count_nonzero(want == 0.0))
    if kind == "ones":  # h = [1, 1]: the sum is exactly +0.0 wherever the two bits differ
        assert 0.4 < zeros / checked < 0.6, (zeros, checked)


# ---------------------------------------------------------------- (b) the noise sample against float64
def noise_errors(z, z_ref, r_ref):
    """(worst |z - z_ref| / r_ref, largest |z - z_ref| and its (b, t)) -- samples with r_ref = 0 must be 0 themselves."""
    err = np.abs(z.astype(np.float64) - z_ref)
    assert np.all(err[r_ref == 0.0] == 0.0)
    rel = np.divide(err, r_ref, out=np.zeros_like(err), where=r_ref > 0.0)
    at = np.unravel_index(np.argmax(err), err.shape)
    return float(rel.max()), float(err.max()), tuple(int(v) for v in at)


def test_noise_sample_against_float64(dev, refs, z_kernel):
    """|z - z_ref| <= TAU r_ref + 2^-149, every sample.  The figures are printed before anything is asserted: TAU is four times the
    worst ratio measured here, rounded up to a power of two (profiles/word_gen_exactness.txt), and at most TAU_MAX = 2^-10."""
    assert R.TAU <= R.TAU_MAX == 2.0 ** -10
    worst, failed = 0.0, []
    for seed in SEEDS:
        for B, T in SHAPES:
            _, z_ref, r_ref = refs(seed, B, T)
            z = z_kernel(seed, B, T)
            rel, err, at = noise_errors(z, z_ref, r_ref)
            worst = max(worst, rel)
            print(f"word_gen noise: seed {seed:#x} B {B} T {T}: worst |z - z_ref| / r_ref = {rel:.4e} = 2^{np.log2(max(rel, 1e-300)):.2f}, "
                  f"largest |z - z_ref| = {err:.4e} at (b, t) = {at} (z_ref {z_ref[at]:+.6f}, r_ref {r_ref[at]:.6f})")
            n_bad = int(np.count_nonzero(np.abs(z.astype(np.float64) - z_ref) > R.TAU * r_ref + 2.0 ** -149))
            if n_bad:
                failed.append((hex(seed), B, T, n_bad))
    need = 2.0 ** np.ceil(np.log2(4 * worst)) if worst > 0 else 0.0
    print(f"word_gen noise: worst ratio over all shapes {worst:.4e}; four times it, rounded up to a power of two: 2^{np.log2(need):.0f}; "
          f"TAU in use 2^{np.log2(R.TAU):.0f}")
    assert not failed, failed
    assert R.TAU >= need, "TAU is less than four times the measured worst, rounded up to a power of two"


# ---------------------------------------------------------------- (c) the composition, exact
@pytest.mark.parametrize("L", (2, 4, 8, 16))
@pytest.mark.parametrize("snr", (9.0, 10.0))
def test_composition_is_exact(dev, refs, z_kernel, snr, L):
    sigma = R.sigma_of(snr)
    h = np.random.RandomState(7 * L).normal(0, 1, (3, L))
    for seed in SEEDS:
        for B, T in SHAPES:
            bits = refs(seed, B, T)[0]
            want = (R.isi_ref(bits, h, L) + sigma * z_kernel(seed, B, T).astype(np.float64)).astype(np.float32)
            tx, y = (t.cpu().numpy() for t in mvn.generate_words(B, T, h, snr, L, dev, seed))
            tag = f"snr {snr} L {L} seed {seed:#x} B {B} T {T}"
            assert np.array_equal(tx, bits.astype(np.float32)), tag
            bad = np.argwhere(bits_of(y) != bits_of(want))
            assert len(bad) == 0, f"{tag}: {len(bad)} samples differ, first (b, t) = {bad[0].tolist()}: {y[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- (d) call shapes
@pytest.mark.parametrize("B,T,L", ((5, 1, 4), (9, 130, 8), (37, 257, 2)))
def test_call_shapes(dev, B, T, L):
    seed, sigma = SEEDS[1], R.sigma_of(9.0)
    h = np.random.RandomState(L).normal(0, 1, (3, L))
    tx, y = generate(dev, seed, B, T, h, sigma, L)
    assert np.array_equal(tx, R.bits_ref(seed, B, T).astype(np.float32))
    # tx = NULL: the same y
    none, y2 = generate(dev, seed, B, T, h, sigma, L, want_tx=False)
    assert none is None and np.array_equal(bits_of(y2), bits_of(y))
    # leading dimensions: the rows land at their strides, the padding columns are untouched
    txp, yp = generate(dev, seed, B, T, h, sigma, L, y_ld=T + 3, tx_ld=T + 5)
    assert yp.shape == (B, T + 3) and txp.shape == (B, T + 5)
    assert np.array_equal(bits_of(yp[:, :T]), bits_of(y)) and np.array_equal(txp[:, :T], tx)
    assert np.all(yp[:, T:] == SENTINEL) and np.all(txp[:, T:] == SENTINEL)
    # a call's words are the first words of any longer call; rows beyond B are not written
    B2 = B + 4
    tx_l, y_l = generate(dev, seed, B2, T, h, sigma, L)
    assert np.array_equal(bits_of(y_l[:B]), bits_of(y)) and np.array_equal(tx_l[:B], tx)
    tx_s, y_s = generate(dev, seed, B, T, h, sigma, L, rows=B2)
    assert np.array_equal(bits_of(y_s[:B]), bits_of(y)) and np.all(y_s[B:] == SENTINEL) and np.all(tx_s[B:] == SENTINEL)
    # empty calls return 0 and write nothing
    for b, t in ((0, T), (B, 0)):
        tx_e, y_e = generate(dev, seed, b, t, h, sigma, L, y_ld=T, tx_ld=T, rows=B)
        assert np.all(y_e == SENTINEL) and np.all(tx_e == SENTINEL)


# ---------------------------------------------------------------- (e) global word indexing through the fused route
def test_fused_route_across_word_index_2_to_32(dev, golden):
    """mvn.vnet_monte_carlo(first_word = 2^32 - 3) over 8 words: its counters are those of the restatement's words word0 .. word0 + 7
    (b_lo wraps, b_hi steps to 1) decoded by val_count.  The words are built on the host from z_ref; the device's differ from them
    by the noise tolerance, so the comparison is exact only where no decision is within that tolerance of flipping: the first of
    R.MC_SEEDS with no such symbol is used (tests/test_word_gen_ref_host.py: the first seed has none on the CPU oracle)."""
    g7 = golden("g7_by_word")
    det = mvn.VNETDetector(16, {"train": R.MC_T, "val": R.MC_T}).to(dev)
    with torch.no_grad():
        for p, k in zip(det.net.parameters(), range(6)):
            p.copy_(torch.from_numpy(g7[f"w{k}"]))
    h = R.MC_TAPS
    decode = lambda a: det(torch.as_tensor(a, device=dev), "val").cpu().numpy()  # noqa: E731
    for seed in R.MC_SEEDS:
        bits, y, y_lo, y_hi = R.mc_case(seed)
        edge = R.knife_edge_symbols(decode, y, y_lo, y_hi)
        print(f"seed {seed}: {int(np.count_nonzero(y_lo != y_hi))} samples with more than one float32 in reach, {edge} decisions on a knife edge")
        if edge == 0:
            break
    else:
        pytest.fail("every seed has a decision within the noise tolerance of flipping")
    want = det.val_count(torch.as_tensor(y, device=dev), torch.as_tensor(bits.astype(np.float32), device=dev)).tolist()
    got = mvn.vnet_monte_carlo(det, R.MC_WORDS, h, R.MC_SNR, dev, seed, first_word=R.MC_WORD0).tolist()
    print(f"seed {seed}: fused route {got}, restated words {want}")
    assert got == want
    assert got[1] == R.MC_WORDS * R.MC_T and got[3] == R.MC_WORDS
    # the split matters: words 3 .. 7 have b_lo = 0 .. 4 and b_hi = 1, and are not words 0 .. 4
    assert not np.array_equal(R.bits_ref(seed, 5, R.MC_T, 0), bits[3:])
