// word_gen.inc -- on-device word generator (SURVEY 8f next #1): the whole of ChannelModelDataset.get_snr_data's inner
// loop for uncoded words (channel_dataset.py:65-83: random bits -> zero padding by L -> BPSK -> ISIAWGNChannel.transmit,
// channel.py:12-35) in ONE kernel, so that at-scale Monte-Carlo runs (10^9 symbols for BASELINE configs[3]) never
// materialise int8 bits, a float cast and a noise tensor (17 B/symbol of HBM traffic in three ATen kernels) to feed a
// detector that reads 4 B/symbol.  Included by mvn_hip.hip inside its anonymous namespace.
//
// Randomness is counter-based (Philox4x32-10, Salmon et al. 2011): bit t of word b and the noise sample of (b, t) are
// pure functions of (seed, b, t), so the result does not depend on the launch geometry and any word can be regenerated
// alone.  The reference draws from two NumPy RandomState streams (MT19937, trainer.py:90-91); this generator has the
// same DISTRIBUTION, not the same stream -- mvn_isi_awgn_transmit stays the bit-exact replay path for recorded draws.
//   bits  : word b, 128-bit group g = t / 128 -> philox(key = seed, counter = (g, b_lo, b_hi, 0)), bit (t % 128),
//           least-significant bit of the .x word first
//   noise : standard normal by Box-Muller on two 32-bit uniforms, 4 samples per philox(key = seed, counter =
//           (t / 4, b_lo, b_hi, 1)) = (x, y, z, w): samples 4q, 4q + 1 = r cos, r sin from (x, y), 4q + 2, 4q + 3 from (z, w).
//           The uniforms are float32 and their ends are reached: u1 = 2^-31 (a/2 + 1/2) lies in [2^-32, 1] ((float)(a >> 1) rounds
//           up to 2^31 from a >> 1 = 2^31 - 64 on, and the + 0.5 is absorbed from 2^23 on), u2 = 2^-32 b lies in [0, 1] ((float)b
//           rounds up to 2^32).  So |z| <= sqrt(-2 ln 2^-32) = sqrt(64 ln 2) ~ 6.67, and z = 0 for the pair when u1 rounds to 1
//           (probability 2^-25); u2 = 1 is the angle 0 again.  Neither end is harmful.
//   tests/word_gen_ref.py restates all of this in NumPy and tests/test_gpu_word_gen.py holds the kernel to it: bits and ISI sum bit
//   for bit, the noise sample to a measured relative error of r (profiles/word_gen_exactness.txt), their composition bit for bit.
//   y[t]  = sum_k h[L-1-k] * s[t+k] + sigma * z, s = 1 - 2 c, c = 0 beyond the word (channel_dataset.py:71): float64
//           accumulation like the reference's NumPy code, stored fp32 (channel_dataset.py:103).

struct Philox4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &z0, float &z1) {
    const float u1 = ((float)(a >> 1) + 0.5f) * 4.656612873077392578125e-10f;  // [2^-32, 1]: 2^-31 * (a/2 + 1/2), rounded
    const float u2 = (float)b * 2.3283064365386962890625e-10f;                   // [0, 1]: (float)b rounds up to 2^32
    const float r = sqrtf(-2.0f * logf(u1));
    z0 = r * __builtin_amdgcn_cosf(u2);  // v_cos_f32 / v_sin_f32 take their argument in revolutions: cos(2 pi u2)
    z1 = r * __builtin_amdgcn_sinf(u2);
}

// Four consecutive received samples y[t0 .. t0 + 3] of word b (t0 % 4 == 0) and its transmitted bits t0 .. t0 + 3 (bit i of
// `txbits`; samples at t >= T are meaningless).  hb: the word's L taps.  The generator kernel and the fused Monte-Carlo detectors
// (va_montecarlo below: "fused into the decode kernel so y never touches HBM", SURVEY 8f#1) share it: the same values, bit for bit.
__device__ __forceinline__ void generate_quad(uint32_t seed_lo, uint32_t seed_hi, int64_t b, int t0, int T, int L, const double *hb,
                                              double sigma, float (&yv)[4], unsigned &txbits) {
    const int K = T;  // one received sample per transmitted bit (channel_dataset.py:71-79)
    const uint32_t b_lo = (uint32_t)b, b_hi = (uint32_t)(b >> 32);
    // bits t0 .. t0 + 3 + L - 1 (L <= 16: at most 19 bits) lie in at most two 128-bit groups: take the 32-bit window that
    // starts at bit t0 of the 256-bit string (group g0, group g0 + 1)
    const int g0 = t0 >> 7;
    const Philox4 p0 = philox4x32_10((uint32_t)g0, b_lo, b_hi, 0u, seed_lo, seed_hi);
    const int wi = (t0 >> 5) & 3, sh = t0 & 31;
    uint32_t next = 0;  // first word of group g0 + 1, needed only by the last word of a group
    if (wi == 3 && sh + 3 + L - 1 >= 32) next = philox4x32_10((uint32_t)(g0 + 1), b_lo, b_hi, 0u, seed_lo, seed_hi).x;
    const uint32_t lo = wi == 0 ? p0.x : wi == 1 ? p0.y : wi == 2 ? p0.z : p0.w;
    const uint32_t hi = wi == 0 ? p0.y : wi == 1 ? p0.z : wi == 2 ? p0.w : next;
    uint32_t win = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    const int left = K - t0;  // bits of the word from t0 on; beyond it the zero padding (channel_dataset.py:71)
    if (left < 32) win &= left > 0 ? (1u << left) - 1u : 0u;
    txbits = win & 15u;
    const Philox4 pn = philox4x32_10((uint32_t)(t0 >> 2), b_lo, b_hi, 1u, seed_lo, seed_hi);
    float z[4];
    box_muller(pn.x, pn.y, z[0], z[1]);
    box_muller(pn.z, pn.w, z[2], z[3]);
    // np.dot(h[:, ::-1], blockwise_s) (channel.py:25-27), same order of accumulation.  The BPSK symbol s = 1 - 2 c (modulator.py:12;
    // padding -> +1) is +-1, so h s is +-h exactly and each term is ONE rounded float64 addition either way -- written as a
    // conditional negation: the 19 symbols as doubles were 38 registers of every kernel that generates its words itself
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < L; ++k) {
        const double hk = hb[L - 1 - k];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += ((win >> (i + k)) & 1u) ? -hk : hk;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) yv[i] = (float)(acc[i] + sigma * (double)z[i]);
}

constexpr int kGenThreads = 256;
// one thread = 4 consecutive received samples of one word
__global__ __launch_bounds__(kGenThreads) void generate_words_kernel(float *__restrict__ tx, int64_t tx_ld, float *__restrict__ y,
                                                                     int64_t y_ld, const double *__restrict__ h, int64_t Bh,
                                                                     double sigma, uint32_t seed_lo, uint32_t seed_hi, int64_t B,
                                                                     int T, int L) {
    const int quads = (T + 3) >> 2;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * quads) return;
    const int64_t b = e / quads;
    const int t0 = 4 * (int)(e % quads);
    float yv[4];
    unsigned txbits;
    generate_quad(seed_lo, seed_hi, b, t0, T, L, h + (b % Bh) * L, sigma, yv, txbits);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + i;
        if (t >= T) break;
        y[b * y_ld + t] = yv[i];
        if (tx) tx[b * tx_ld + t] = (float)((txbits >> i) & 1u);
    }
}
