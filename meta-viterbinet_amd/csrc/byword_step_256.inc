// byword_step_256.inc -- the by-word block step (byword_step.inc) at 256 states, channel memory 8 (included by mvn_hip.hip after
// byword_step_states_va.inc): mvn_vnet_byword_step_256_f32 / mvn_vnet_byword_step_256_path_f32 for the ViterbiNet detector and
// mvn_va_byword_step_256_f32 / mvn_va_byword_step_256_path_f32 for the classical one.
//
// The frame is byword_step_states.inc's -- one workgroup of kStatesWaves waves per word, an LDS image [t][S] of logits (ViterbiNet) or
// of -va_cost (classical), ONE wave for the sweep, which carries on into byword_codec -- and the codec, rs_generator_poly, the pilot
// step, StepOut and WeightStrides are that family's, called as they stand.  That family cannot be instantiated here: its sweep holds at
// most two states per lane, and next to the 53 KB W3 image a whole word [T][256] at 1 KB per symbol stops near 96 symbols, below the
// reference's 136.  So three things are this file's own; StatesCfg, states_sweep_word and states_path_word are not touched.
//   segments  the word goes through the LDS kStep256Seg symbols at a time (step256_seg<VA>(): a multiple of 16, what the LDS holds
//             next to the static part and the path step's survivors).  Per segment: the producers fill image[i][256], i < len; barrier;
//             wave 0 sweeps the rows, the path metrics staying in its registers from one segment to the next; barrier; the next
//             segment.  The number of segments depends on T alone and every wave passes every barrier: wave 0 and the others run
//             DIFFERENT loops with the SAME barrier count (ViterbiNet), or one loop (classical).  Production and sweep do NOT overlap:
//             two half buffers would halve the segment and double the barriers of the reference's word.
//             ViterbiNet: waves 1 .. 7 take the segment's 16-symbol tiles round-robin through mlp_stage_w3<16> / mlp_load_weights /
//             mlp_tile<16> -- mlp_kernel's code, so the logits are mvn_vnet_logits_f32's bit for bit.  Wave 0 takes no tile: the
//             200 VGPRs of layer-1 and layer-2 weights would otherwise stay live over its sweep.
//             Classical: states_va_costs<256> (byword_step_states_va.inc) by all eight waves, the priors of row r % Bp.
//   sweep     state s = l + 64 r lives in lane l, register r (0 .. 3).  Its predecessors 2 s mod 256 and 2 s + 1 mod 256 sit in lanes
//             2 l mod 64 and 2 l + 1 mod 64, register (l >= 32) + 2 (r & 1): registers r and r + 2 end every stage with one value,
//             128 distinct metrics, two per lane (m[r & 1]).  Candidates a = m + -image[t][s], torch.min's ACS (min2_torch_dev; the
//             lone wave always runs the NaN-propagating stage: no guard launch).
//   running   the decision of symbol t is torch.argmin of the metrics BEFORE stage t (quirk Q1), % 2: the first minimum, a NaN
//             minimal.  States s and s + 128 hold one value, so the argmin never lands in the upper half, and of a lane's two metrics
//             the upper one (state l + 64) wins only when it is strictly smaller.  The lane puts its winner back over row t as ONE
//             64-bit word, step256_key(metric) above the state index: an unsigned order in which NaN is 0, -0 equals +0 and every other
//             value keeps its place, so the smallest word of the row IS torch.argmin's (value, index) pair.  A lane per symbol then
//             takes the minimum of its row's 64 words.
//   path      torch.min's index as sweep_surv_kernel defines it, second = !(v1 >= v0) && v0 == v0: 128 distinct bits per stage, two
//             ballots, four dwords -- bit (sigma & 31) of dword (sigma >> 5) & 3 is state sigma's -- in an array of the word's own
//             after the image (16 B per stage: the rows do not survive the next segment).  Then torch.argmin of the final metrics and
//             the walk s = (2 s + j) & 255 over the whole word, 32 stages per load as in states_path_word.
constexpr int kStep256States = 256;
constexpr int kStep256MaxT = kCoopMaxT;  // StepShared's images; the codec's root search covers 128 bytes
constexpr int kStep256SurvBytes = 16;    // a stage's survivors

template <int NS>
struct Step256Shared : StepShared<NS> {
    __attribute__((aligned(16))) float a3[16 * kK3Steps * 64];  // W3 in A-operand order (mlp_stage_w3)
    float b3[kStep256States];
};

// the symbols of one segment: what the LDS holds next to the larger (NS = 8) static part and the longest word's survivors
template <bool VA>
constexpr int step256_seg() {
    constexpr size_t fixed = ((VA ? sizeof(StepShared<8>) : sizeof(Step256Shared<8>)) + 15) / 16 * 16;
    constexpr size_t surv = (size_t)kStep256MaxT * kStep256SurvBytes;
    static_assert(fixed + surv + 16 * 4 * kStep256States <= kStatesLdsBytes, "no room for one tile");
    return (int)((kStatesLdsBytes - fixed - surv) / (4 * (size_t)kStep256States) / 16 * 16);
}

// the dynamic LDS of a data step on T symbols: the rows of one segment (a shorter word: of its tiles), then the path's survivors
template <bool VA>
constexpr size_t step256_dynamic_lds(int T, bool path) {
    const int rows = (T + 15) / 16 * 16 < step256_seg<VA>() ? (T + 15) / 16 * 16 : step256_seg<VA>();
    return (size_t)rows * 4 * kStep256States + (path ? (size_t)T * kStep256SurvBytes : 0);
}

// torch.argmin's order on fp32 as an unsigned key: NaN -> 0 (minimal, whatever its sign bit), -0 -> +0's key, and a < b <=> key(a) <
// key(b) for every other pair (a negative value's bits are inverted, a positive one's get the top bit)
__device__ __forceinline__ unsigned step256_key(float v) {
    const unsigned raw = __float_as_uint(v), b = raw == 0x80000000u ? 0u : raw;
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return v != v ? 0u : k;
}

// One segment by ONE wave: rows image[i][256], i < len (a multiple of 8), are stages t0 .. t0 + len - 1 of the word; m: the metric of
// states lane + 64 rho (and lane + 64 rho + 128) before stage t0, after stage t0 + len - 1 on return.  PATH: stage t's survivors to
// surv[4 t .. 4 t + 3]; else the lane's (key, state) word of the metrics before stage t0 + i over image[i][2 lane .. 2 lane + 1].
template <bool PATH>
__device__ __forceinline__ void step256_sweep_segment(float *image, int len, int t0, int lane, float (&m)[2], unsigned *surv) {
    constexpr int S = kStep256States, TC = 8;
    const int src0 = (2 * lane) & 63, src1 = src0 + 1;  // the lanes that hold states 2 s mod 256 and 2 s + 1 mod 256
    const bool up = lane >= 32;                         // ... in the odd register of the pair
    auto load_chunk = [&](int i0, float (&c)[TC][4]) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) c[i][r] = image[(i0 + i) * S + lane + 64 * r];
    };
    float cur[TC][4], nxt[TC][4];
    load_chunk(0, nxt);
    for (int i0 = 0; i0 < len; i0 += TC) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[i][r] = nxt[i][r];
        if (i0 + TC < len) load_chunk(i0 + TC, nxt);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            float a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = m[r & 1] + -cur[i][r];
            if constexpr (!PATH) {
                // the metrics before stage t0 + i0 + i, what its decision is taken from: the lane's smaller one (the first of two equals)
                const unsigned k0 = step256_key(m[0]), k1 = step256_key(m[1]);
                const bool upper = k1 < k0;
                uint2 w;
                w.x = upper ? (unsigned)lane + 64u : (unsigned)lane;  // (little endian: the key is the word's upper half)
                w.y = upper ? k1 : k0;
                *reinterpret_cast<uint2 *>(image + (i0 + i) * S + 2 * lane) = w;
            }
            unsigned long long bal[2];
#pragma unroll
            for (int rho = 0; rho < 2; ++rho) {
                const float l0 = __shfl(a[2 * rho], src0), l1 = __shfl(a[2 * rho], src1);
                const float h0 = __shfl(a[2 * rho + 1], src0), h1 = __shfl(a[2 * rho + 1], src1);
                const float v0 = up ? h0 : l0, v1 = up ? h1 : l1;
                if constexpr (PATH) {
                    const bool second = !(v1 >= v0) && v0 == v0;  // torch.min(dim): the first minimal index, the first NaN
                    bal[rho] = __ballot(second);
                }
                m[rho] = min2_torch_dev(v0, v1);
            }
            if constexpr (PATH) {
                if (lane == 0) {
                    uint4 w;
                    w.x = (unsigned)bal[0];
                    w.y = (unsigned)(bal[0] >> 32);
                    w.z = (unsigned)bal[1];
                    w.w = (unsigned)(bal[1] >> 32);
                    *reinterpret_cast<uint4 *>(surv + 4 * (t0 + i0 + i)) = w;
                }
            }
        }
    }
    wave_lds_fence();
}

// the running decisions of a segment that step256_sweep_segment<false> has swept: one lane per symbol takes the smallest of its row's
// 64 (key, state) words -- torch.argmin: the first minimum, a NaN minimal -- and sink(t, state % 2).  The lanes start at different
// words: their reads spread over the banks.
template <class Sink>
__device__ __forceinline__ void step256_decide_segment(const float *image, int len, int t0, int lane, Sink sink) {
    constexpr int S = kStep256States;
    for (int i = lane; i < len; i += 64) {
        const unsigned long long *row = reinterpret_cast<const unsigned long long *>(image + i * S);
        unsigned long long best = row[lane];
#pragma unroll 8
        for (int e = 1; e < 64; ++e) {
            const unsigned long long o = row[(e + lane) & 63];
            best = o < best ? o : best;
        }
        sink(t0 + i, (float)((unsigned)best & 1u));
    }
}

// The traced-back path of the whole word by ONE wave, after its last segment: sigma_T = torch.argmin of the final metrics (the first
// minimum, a NaN minimal, the lower index among equals; states s + 128 repeat states s and never win), then for t = T - 1 ... 0:
// j = state sigma's survivor of stage t, sigma = (2 sigma + j) mod 256, bit[t] = sigma & 1 (mvn_traceback_f32's bits).  32 stages are
// ONE 16-byte load, a stage per lane, requested before the 32 stages above them are walked; the walk is scalar arithmetic.
__device__ __forceinline__ void step256_walk_word(const unsigned *surv, const float (&m)[2], int T, int lane, unsigned char *dbits,
                                                  float *__restrict__ dec) {
    constexpr int S = kStep256States, WK = 32;
    int s;
    {
        float bv = m[0];
        int bi = lane;
        {
            const float ov = m[1];
            const int oi = lane + 64;
            const bool onan = ov != ov, bnan = bv != bv;
            const bool take = onan ? !bnan : (!bnan && ov < bv);  // (oi > bi: a tie stays)
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            const bool onan = ov != ov, bnan = bv != bv;
            const bool take = onan ? (!bnan || oi < bi) : (!bnan && ((ov < bv) || (ov == bv && oi < bi)));
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        s = __builtin_amdgcn_readfirstlane(bi);
    }
    // lane l's survivors of the 32 stages from `base`: stage base + (l & 31); a stage below 0 walks zeros, its bit is not stored
    auto fetch = [&](int base, uint4 &w) {
        const int t = base + (lane & (WK - 1));
        w = make_uint4(0u, 0u, 0u, 0u);
        if (t >= 0) w = *reinterpret_cast<const uint4 *>(surv + 4 * t);
    };
    uint4 c, nx;
    fetch(T - WK, c);
    for (int base = T - WK; base > -WK; base -= WK) {
        fetch(base - WK, nx);
        unsigned path = 0;  // bit e: symbol base + e
#pragma unroll
        for (int e = WK - 1; e >= 0; --e) {
            const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)c.x, e), w1 = (unsigned)__builtin_amdgcn_readlane((int)c.y, e);
            const unsigned w2 = (unsigned)__builtin_amdgcn_readlane((int)c.z, e), w3 = (unsigned)__builtin_amdgcn_readlane((int)c.w, e);
            const unsigned w = (s & 64) ? ((s & 32) ? w3 : w2) : ((s & 32) ? w1 : w0);
            const int j = (int)(w >> (s & 31)) & 1;
            s = (2 * s + j) & (S - 1);
            path |= (unsigned)(s & 1) << e;
        }
        const int t = base + lane;
        if (lane < WK && t >= 0) {
            const int bit = (int)(path >> lane) & 1;
            dbits[t] = (unsigned char)bit;
            if (dec) dec[t] = (float)bit;
        }
        c = nx;
    }
}

// The ViterbiNet kernels' staging and segment loop, ONE copy as text (MVN_STATES_PHASE1's reasons): it expands in the kernel's body and
// reads its parameters and its locals sh, image, r, lane, wave by name.  SWEEP(len, t0): what wave 0 makes of a produced segment.
// Barriers: one after the staging; then per segment one before its production (from the second segment on: wave 0 has left the
// rows) and one after it.  Waves 1 .. 7 run the first loop and return, wave 0 the second: the same count in both, a function of T.
#define MVN_STEP256_VNET_SEGMENTS(DATA, SWEEP)                                                                                   \
    constexpr int SEG = step256_seg<false>();                                                                                    \
    const int nseg = (DATA) ? (T + SEG - 1) / SEG : 0;                                                                           \
    if (DATA) mlp_stage_w3<16>(sh.a3, sh.b3, W3 + r * ws.s[4], b3 + r * ws.s[5], kStep256States);                                \
    __syncthreads();                                                                                                             \
    if (wave != 0) {                                                                                                             \
        if (nseg == 0) return;                                                                                                   \
        const int j = lane & 15, q = lane >> 4;                                                                                  \
        const float *rxb = rx + r * rx_ld;                                                                                       \
        float nw1[kK2Steps], nb1[kK2Steps], a2[4][kK2Steps], b2v[4][4];                                                          \
        mlp_load_weights(W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2], b2 + r * ws.s[3], j, q, nw1, nb1, a2, b2v);       \
        for (int seg = 0; seg < nseg; ++seg) {                                                                                   \
            const int t0 = seg * SEG, len = T - t0 < SEG ? T - t0 : SEG;                                                         \
            if (seg) __syncthreads();                                                                                            \
            const int ntiles = (len + 15) >> 4;                                                                                  \
            for (int tile = wave - 1; tile < ntiles; tile += kStatesWaves - 1) {                                                 \
                const int i = 16 * tile + j, t = t0 + i;                                                                         \
                const float yj = rxb[t < T ? t : T - 1];                                                                         \
                mlp_tile<16>(yj, nw1, nb1, a2, b2v, sh.a3, lane, [&](int j3, f32x4 acc3) {                                       \
                    const int st0 = 16 * j3 + 4 * q;                                                                             \
                    if (i < len) {                                                                                               \
                        float4 v;                                                                                                \
                        v.x = acc3[0] + sh.b3[st0 + 0];                                                                          \
                        v.y = acc3[1] + sh.b3[st0 + 1];                                                                          \
                        v.z = acc3[2] + sh.b3[st0 + 2];                                                                          \
                        v.w = acc3[3] + sh.b3[st0 + 3];                                                                          \
                        *reinterpret_cast<float4 *>(&image[i * kStep256States + st0]) = v;                                       \
                    }                                                                                                            \
                });                                                                                                              \
            }                                                                                                                    \
            __syncthreads();                                                                                                     \
        }                                                                                                                        \
        return;                                                                                                                  \
    }                                                                                                                            \
    for (int seg = 0; seg < nseg; ++seg) {                                                                                       \
        const int t0 = seg * SEG, len = T - t0 < SEG ? T - t0 : SEG;                                                             \
        if (seg) __syncthreads();                                                                                                \
        __syncthreads();                                                                                                         \
        SWEEP(len, t0);                                                                                                          \
    }

// The classical kernels' loop: all eight waves produce a segment, wave 0 sweeps it.
#define MVN_STEP256_VA_SEGMENTS(DATA, SWEEP)                                                                                     \
    constexpr int SEG = step256_seg<true>();                                                                                     \
    const int nseg = (DATA) ? (T + SEG - 1) / SEG : 0;                                                                           \
    for (int seg = 0; seg < nseg; ++seg) {                                                                                       \
        const int t0 = seg * SEG, len = T - t0 < SEG ? T - t0 : SEG;                                                             \
        if (seg) __syncthreads();                                                                                                \
        states_va_costs<kStep256States>(image, rx + r * rx_ld + t0, priors + (r % Bp) * kStep256States, len);                    \
        __syncthreads();                                                                                                         \
        if (wave == 0) SWEEP(len, t0);                                                                                           \
    }                                                                                                                            \
    if (nseg == 0) __syncthreads();                                                                                              \
    if (wave != 0) return;

template <int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_step_256_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    __shared__ Step256Shared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float image[];  // logit[i][256], i < SEG: one segment (a data step's)
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    float m[2] = {0.0f, 0.0f};  // vnet_detector.py: in_prob starts at zero
    float *decb = dec ? dec + r * dec_ld : nullptr;
    unsigned char *dbits = sh.dbits;
#define MVN_STEP256_SWEEP(len, t0)                                                   \
    {                                                                                \
        step256_sweep_segment<false>(image, len, t0, lane, m, nullptr);              \
        step256_decide_segment(image, len, t0, lane, [&](int t, float mydec) {       \
            if (decb) decb[t] = mydec;                                               \
            dbits[t] = (unsigned char)mydec;                                         \
        });                                                                          \
    }
    MVN_STEP256_VNET_SEGMENTS(!pilot, MVN_STEP256_SWEEP)
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, 8>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}

template <int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_step_256_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    __shared__ StepShared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float image[];  // -cost[i][256], i < SEG: one segment (a data step's)
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    float m[2] = {0.0f, 0.0f};
    float *decb = dec ? dec + r * dec_ld : nullptr;
    unsigned char *dbits = sh.dbits;
    MVN_STEP256_VA_SEGMENTS(!pilot, MVN_STEP256_SWEEP)
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, 8>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}
#undef MVN_STEP256_SWEEP

// ---- The same steps on the TRACED-BACK PATH: data steps; the image is followed by the word's survivors, 16 B per stage.
#define MVN_STEP256_SWEEP(len, t0) step256_sweep_segment<true>(image, len, t0, lane, m, surv)

template <int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_path_step_256_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym) {
    __shared__ Step256Shared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float image[];  // logit[i][256], i < SEG; then the survivors of the T stages
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    float m[2] = {0.0f, 0.0f};
    unsigned *surv = reinterpret_cast<unsigned *>(image + (step256_dynamic_lds<false>(T, false) >> 2));
    MVN_STEP256_VNET_SEGMENTS(true, MVN_STEP256_SWEEP)
    step256_walk_word(surv, m, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, 8>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}

template <int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_path_step_256_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym) {
    __shared__ StepShared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float image[];  // -cost[i][256], i < SEG; then the survivors of the T stages
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    float m[2] = {0.0f, 0.0f};
    unsigned *surv = reinterpret_cast<unsigned *>(image + (step256_dynamic_lds<true>(T, false) >> 2));
    MVN_STEP256_VA_SEGMENTS(true, MVN_STEP256_SWEEP)
    step256_walk_word(surv, m, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, 8>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}
#undef MVN_STEP256_SWEEP
#undef MVN_STEP256_VNET_SEGMENTS
#undef MVN_STEP256_VA_SEGMENTS
