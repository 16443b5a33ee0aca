"""The on-device word generator (csrc/word_gen.inc: generate_quad, shared by mvn_generate_words_f32 and the one-launch Monte-Carlo
kernels) restated in NumPy, as its referee: plain functions of (seed, word, position), no GPU, nothing taken from a kernel.

  bits   word b, 128-bit group g = t // 128: philox(key = seed, counter = (g, b_lo, b_hi, 0)), bit t % 128, least-significant bit of
         the first word first
  noise  word b, quad q = t // 4: philox(key = seed, counter = (q, b_lo, b_hi, 1)) = (x, y, z, w); Box-Muller on (x, y) gives samples
         4q and 4q + 1, on (z, w) samples 4q + 2 and 4q + 3.  The two uniforms are the kernel's float32 values, reproduced bit for bit
         (three IEEE operations each, the library is built with -ffp-contract=off and without fast-math); everything after them is
         float64 here and float32 (logf, sqrtf, v_cos_f32 / v_sin_f32) on the device -- the one place a tolerance is needed
  isi    acc = sum_k +-h[b % Bh, L-1-k], k = 0 .. L-1 in this order in float64, minus where bit t + k is 1; bits at or beyond T are 0

tests/test_word_gen_ref_host.py checks these functions on the CPU; tests/test_gpu_word_gen.py holds the kernels to them."""
import numpy as np

M32 = 0xFFFFFFFF
R_MAX = float(np.sqrt(64 * np.log(2.0)))  # sqrt(-2 ln 2^-32): the largest Box-Muller radius, ~6.6604


def philox4x32_10(c, k):
    """NumPy Philox4x32-10 (Salmon et al. 2011; Random123): c [n,4] uint32 counters, k (k0, k1) -> [n,4] uint32."""
    c = c.astype(np.uint64)
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    M0, M1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]
        c = np.stack([(p1 >> np.uint64(32)) ^ c[:, 1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[:, 3] ^ k1, p0 & MASK], axis=1)
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return c.astype(np.uint32)


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & M32, seed >> 32


def _words(seed, B, n, word0, stream):
    """philox(key = seed, counter = (i, b_lo, b_hi, stream)) for words word0 .. word0 + B - 1 and i = 0 .. n - 1: uint32 [B, n, 4]."""
    b = [int(word0) + i for i in range(B)]  # Python integers: word indices above 2^32
    ctr = np.empty((B, n, 4), np.uint64)
    ctr[:, :, 0] = np.arange(n, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = np.array([v & M32 for v in b], np.uint64)[:, None]
    ctr[:, :, 2] = np.array([v >> 32 for v in b], np.uint64)[:, None]
    ctr[:, :, 3] = stream
    return philox4x32_10(ctr.reshape(B * n, 4).astype(np.uint32), _key(seed)).reshape(B, n, 4)


def bits_ref(seed, B, T, word0=0):
    """The transmitted bits of words word0 .. word0 + B - 1: uint8 [B, T]."""
    groups = (T + 127) // 128
    w = _words(seed, B, groups, word0, 0).reshape(B, groups * 4)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(B, groups * 128)[:, :T].astype(np.uint8)


def u1_ref(a):
    """The radius uniform of a 32-bit word, in the kernel's float32 operations: in [2^-32, 1] (a >> 1 rounds up to 2^31 from
    2^31 - 64 on, and the + 0.5 is absorbed from 2^23 on)."""
    a = np.asarray(a, np.uint32)
    return ((a >> np.uint32(1)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -31)


def u2_ref(b):
    """The angle uniform of a 32-bit word, in revolutions, in the kernel's float32 operations: in [0, 1] (b rounds up to 2^32 from
    2^32 - 128 on)."""
    return np.asarray(b, np.uint32).astype(np.float32) * np.float32(2.0 ** -32)


def box_muller_ref(a, b):
    """(z0, z1, r) in float64 from the float32 uniforms of the words (a, b)."""
    u1, u2 = u1_ref(a).astype(np.float64), u2_ref(b).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2), r


def noise_ref(seed, B, T, word0=0):
    """(z_ref, r_ref), float64 [B, T]: the standard-normal sample of (word, position) and the Box-Muller radius it was made from
    (the scale of the device's rounding error)."""
    quads = (T + 3) // 4
    w = _words(seed, B, quads, word0, 1)
    z = np.empty((B, quads, 4), np.float64)
    r = np.empty((B, quads, 4), np.float64)
    z[:, :, 0], z[:, :, 1], r[:, :, 0] = box_muller_ref(w[:, :, 0], w[:, :, 1])
    z[:, :, 2], z[:, :, 3], r[:, :, 2] = box_muller_ref(w[:, :, 2], w[:, :, 3])
    r[:, :, 1], r[:, :, 3] = r[:, :, 0], r[:, :, 2]
    return z.reshape(B, quads * 4)[:, :T].copy(), r.reshape(B, quads * 4)[:, :T].copy()


def isi_ref(bits, h, L):
    """The noise-free received words of `bits` [B, T] over the taps h [Bh, L] (row b % Bh for word b): float64 [B, T]."""
    bits = np.asarray(bits)
    B, T = bits.shape
    h = np.asarray(h, np.float64).reshape(-1, L)
    hb = h[np.arange(B) % h.shape[0]]  # [B, L]
    c = np.zeros((B, T + L), bool)
    c[:, :T] = bits != 0
    acc = np.zeros((B, T), np.float64)
    for k in range(L):
        hk = hb[:, L - 1 - k][:, None]
        acc = acc + np.where(c[:, k:k + T], -hk, hk)
    return acc


def sigma_of(snr):
    """The noise standard deviation as the wrappers compute it (channel.py:23,31)."""
    return (10 ** (snr / 10)) ** (-0.5)


# The device's float32 Box-Muller against noise_ref: |z - z_ref| <= TAU r_ref.  MEASURED on the MI355X against this restatement
# (profiles/word_gen_exactness.txt: four times the worst |z - z_ref| / r_ref seen, rounded up to a power of two), and bounded by
# TAU_MAX whatever is measured: an amplitude error of 2^-10 moves the effective SNR by 0.0085 dB, and every structural error (a wrong
# counter, a swapped pair, sin for cos, radians for revolutions) is of the order of r.
TAU_MAX = 2.0 ** -10
TAU = 2.0 ** -20  # measured worst 2.33e-07 = 2^-22.03 (seed 0x0123456789ABCDEF, 300 x 257); four times it is 9.32e-07 <= 2^-20

# The fused Monte-Carlo route's case across word index 2^32 (test_gpu_word_gen.py (e)): 8 words of 40 symbols from word 2^32 - 3 on,
# at 6 dB; the first of these seeds at which no decision is within the noise tolerance of flipping is used.
MC_WORD0, MC_WORDS, MC_T, MC_SNR = 2 ** 32 - 3, 8, 40, 6.0
MC_SEEDS = (20260711, 20260712, 20260713, 20260714, 20260715)
MC_TAPS = np.exp(-0.2 * np.arange(4)).reshape(1, 4) * np.array([[1.0], [0.9], [0.8]])  # three rows, which do not divide 2^32 - 3


def mc_case(seed, tau=None):
    """(bits uint8 [8, 40], y, y_lo, y_hi float32 [8, 40]) of the case above over MC_TAPS (word w uses row w % 3, w the GLOBAL
    index): y = float32(isi + sigma z_ref), and [y_lo, y_hi] holds every float32 the device can give when its noise sample is
    within tau r_ref of z_ref (rounding to float32 is monotone)."""
    tau = TAU if tau is None else tau
    h, L = MC_TAPS, 4
    rows = h[[(MC_WORD0 + i) % h.shape[0] for i in range(MC_WORDS)]]  # one row per word: isi_ref's b % Bh is then b
    bits = bits_ref(seed, MC_WORDS, MC_T, MC_WORD0)
    z, r = noise_ref(seed, MC_WORDS, MC_T, MC_WORD0)
    sigma = sigma_of(MC_SNR)
    clean = isi_ref(bits, rows, L)
    y = clean + sigma * z
    d = tau * sigma * r + 2.0 ** -149
    return bits, y.astype(np.float32), (y - d).astype(np.float32), (y + d).astype(np.float32)


def knife_edge_symbols(decode, y, y_lo, y_hi):
    """The number of symbols whose decision differs between y and either end of its tolerance interval (decode: float32 [B, T] ->
    decisions [B, T]); 0 without decoding when the interval is a single float32 everywhere."""
    if np.array_equal(y_lo, y_hi):
        return 0
    base = np.asarray(decode(y))
    return int(np.count_nonzero((np.asarray(decode(y_lo)) != base) | (np.asarray(decode(y_hi)) != base)))
