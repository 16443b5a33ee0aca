// byword_step_states.inc -- the by-word block step (byword_step.inc) for the ViterbiNet detector at 4, 8, 32, 64 and 128 states
// (included by mvn_hip.hip after byword_step.inc): mvn_vnet_byword_step_states_f32 (the running decision) and, at the end of the
// file, mvn_vnet_byword_step_states_path_f32 (the traced-back path).
//
// Same step, same outputs, one workgroup per word with the word's own weights (WeightStrides); the detector is the two-kernel route
// of these state counts folded into the workgroup:
//   phase 1  the waves take the word's 16-symbol tiles round-robin through mlp_tile (mvn_hip.hip: mlp_kernel's tile, the same code,
//            so the logits are mvn_vnet_logits_f32's bit for bit) and leave them in an LDS image logit[t][S];
//   phase 2  after one barrier wave 0 runs sweep_kernel<S, MODE_NEGLOGIT>'s recurrence from the image: a state per lane (two at 128
//            states), branch cost -logit, torch.min's ACS (min2_torch_dev: NaN when either candidate is), the metrics before every
//            stage left in the image; then the decision of symbol t = argmin_s(metric before stage t) % 2 (quirk Q1: taken BEFORE
//            stage t is absorbed) in torch.argmin's order (first minimum, NaN minimal), a symbol per lane.
//            The lone wave waits for its own cross-lane round trips, not for the minimum: it always runs the NaN-propagating stage,
//            there is no guard;
//   codec    the same wave carries on into byword_codec with the trellis memory log2 S in the label states.
// A pilot step detects nothing (byword_step_kernel's pilot: tables, the transmitted bytes, wave 0 into the codec).
// Eight waves: the tile holds 200 VGPRs of layer-1 and layer-2 weights like mlp_kernel, two waves per SIMD leave it 256.
// LDS: the step's state, the W3 image (13 x 64 floats per 16 states: 26 KB at 128 states) and b3 are static; the
// logit image is dynamic, 4 S bytes per symbol, and bounds the word: states_max_symbols<S>() is the ONE place that says how long.
constexpr int kStatesWaves = 8;
constexpr size_t kStatesLdsBytes = 160 * 1024;  // a CU's LDS

template <int S>
struct StatesCfg {
    static_assert(S >= 4 && S <= 128 && (S & (S - 1)) == 0 && S != 16, "16 states: byword_step_kernel");
    static constexpr int NT3 = (S + 15) / 16;    // 16-state tiles of layer 3
    static constexpr int LPB = S < 64 ? S : 64;  // lanes that hold the word's states
    static constexpr int R = S / LPB;            // states per lane
    static constexpr int MEM = S == 4 ? 2 : S == 8 ? 3 : S == 32 ? 5 : S == 64 ? 6 : 7;  // memory_length: S = 2^MEM
};

template <int S, int NS>
struct StatesStepShared : StepShared<NS> {
    __attribute__((aligned(16))) float a3[StatesCfg<S>::NT3 * kK3Steps * 64];  // W3 in A-operand order (mlp_stage_w3)
    float b3[StatesCfg<S>::NT3 * 16];
};

// Phase 1 of the three kernels of this family (the running and the path step below, the list step of byword_list_states.inc): the
// word's tiles, round-robin over the waves, into states_logit[t][S].  ONE copy as TEXT, and only as text: it expands in the kernel's
// own body and reads the kernel's parameters rx, rx_ld, W1 .. b3, ws, T and its locals C, sh, states_logit, r, lane, wave by name, so
// the compiler sees the lines where they always stood.  A __forceinline__ function around them changes the emitted code of all thirty
// kernels (tools/kernel_isa_diff.py: scalar address arithmetic and the schedule of the tile phase, in the first ~1 800 lines of
// each) -- with the pointers offset at the call; with raw pointers, WeightStrides by value and r, offset inside in the original order;
// and the same with __restrict__ parameters.  byword_step.inc's rule is unchanged code, so none of them was taken.
#define MVN_STATES_PHASE1()                                                                                                      \
    {                                                                                                                            \
        const int j = lane & 15, q = lane >> 4;                                                                                  \
        const float *rxb = rx + r * rx_ld;                                                                                       \
        mlp_stage_w3<C::NT3>(sh.a3, sh.b3, W3 + r * ws.s[4], b3 + r * ws.s[5], S);                                               \
        float nw1[kK2Steps], nb1[kK2Steps], a2[4][kK2Steps], b2v[4][4];                                                          \
        mlp_load_weights(W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2], b2 + r * ws.s[3], j, q, nw1, nb1, a2, b2v);       \
        __syncthreads();                                                                                                         \
        const int ntiles = (T + 15) >> 4;                                                                                        \
        for (int tile = wave; tile < ntiles; tile += kStatesWaves) {                                                             \
            const int t = 16 * tile + j;                                                                                         \
            const float yj = rxb[t < T ? t : T - 1];                                                                             \
            mlp_tile<C::NT3>(yj, nw1, nb1, a2, b2v, sh.a3, lane, [&](int j3, f32x4 acc3) {                                       \
                const int st0 = 16 * j3 + 4 * q;                                                                                 \
                if (st0 < S && t < T) { /* (S is a multiple of 4: the lane's four states are all the trellis's or none) */       \
                    float4 v;                                                                                                    \
                    v.x = acc3[0] + sh.b3[st0 + 0];                                                                              \
                    v.y = acc3[1] + sh.b3[st0 + 1];                                                                              \
                    v.z = acc3[2] + sh.b3[st0 + 2];                                                                              \
                    v.w = acc3[3] + sh.b3[st0 + 3];                                                                              \
                    *reinterpret_cast<float4 *>(&states_logit[t * S + st0]) = v;                                                 \
                }                                                                                                                \
            });                                                                                                                  \
        }                                                                                                                        \
    }

// the longest word the step serves at S states: what the LDS holds next to the larger (NS = 8) static part, in whole bytes of
// eight symbols, and no more than the step's own limit (StepShared's images)
template <int S>
constexpr int states_max_symbols() {
    constexpr size_t fixed = (sizeof(StatesStepShared<S, 8>) + 15) / 16 * 16;
    static_assert(fixed < kStatesLdsBytes, "the static part alone fills the LDS");
    constexpr size_t t = (kStatesLdsBytes - fixed) / (4 * (size_t)S) / 8 * 8;
    return t < (size_t)kCoopMaxT ? (int)t : kCoopMaxT;
}

// Phase 2 by ONE wave, in two parts.  The recurrence: sweep_kernel<S, MODE_NEGLOGIT>'s ACS stage for one word, the logits read from
// the LDS image eight symbols ahead (T is a multiple of 8: no ragged chunk), the two predecessors of a state fetched from their lanes
// (states s and s + S / 2 have the same predecessors 2 s mod S and 2 s + 1 mod S, so at 128 states a lane's two states end every stage
// with one value).  Nothing in the chain waits for a decision: the metric BEFORE stage t overwrites logit[t][.], which the wave already
// holds in registers.  The decisions: one lane per symbol takes torch.argmin of its row of the image -- the first minimum, a NaN
// minimal, as an order on (value, index) pairs, so the lanes may start at different states (their reads spread over the banks) -- and
// sink(t, decision).  At S < 64 the wave's 64 / S lane groups all run the recurrence: same values, same addresses.
template <int S, class Sink>
__device__ __forceinline__ void states_sweep_word(float *image, int T, int lane, Sink sink) {
    using C = StatesCfg<S>;
    constexpr int LPB = C::LPB, R = C::R, TC = 8;
    const int sl = lane % LPB;
    const int src0 = (2 * sl) % LPB, src1 = src0 + 1;  // the lanes that hold states 2 s mod S and 2 s + 1 mod S (R = 2: in register sl >= 32)
    float m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = 0.0f;  // vnet_detector.py: in_prob starts at zero
    auto load_chunk = [&](int t0, float (&c)[TC][R]) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) c[i][r] = image[(t0 + i) * S + sl + LPB * r];
    };
    float cur[TC][R], nxt[TC][R];
    load_chunk(0, nxt);
    for (int t0 = 0; t0 < T; t0 += TC) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) cur[i][r] = nxt[i][r];
        if (t0 + TC < T) load_chunk(t0 + TC, nxt);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            float a[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                image[(t0 + i) * S + sl + LPB * r] = m[r];  // the metric before stage t0 + i: what its decision is taken from
                a[r] = m[r] + -cur[i][r];
            }
            float v0 = __shfl(a[0], src0), v1 = __shfl(a[0], src1);
            if (R == 2) {
                const float w0 = __shfl(a[R - 1], src0), w1 = __shfl(a[R - 1], src1);
                v0 = sl < 32 ? v0 : w0;
                v1 = sl < 32 ? v1 : w1;
            }
            const float mn = min2_torch_dev(v0, v1);
#pragma unroll
            for (int r = 0; r < R; ++r) m[r] = mn;
        }
    }
    wave_lds_fence();
    for (int t = lane; t < T; t += 64) {
        const float *row = image + t * S;
        int bi = lane & (S - 1);
        float bv = row[bi];
#pragma unroll 8
        for (int i = 1; i < S; ++i) {
            const int oi = (i + lane) & (S - 1);
            const float ov = row[oi];
            // torch.argmin order: NaN sorts before everything, ties (and NaN vs NaN) go to the lower index
            const bool onan = ov != ov, bnan = bv != bv;
            const bool take = onan ? (!bnan || oi < bi) : (!bnan && ((ov < bv) || (ov == bv && oi < bi)));
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        sink(t, (float)(bi & 1));
    }
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_step_states_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    using C = StatesCfg<S>;
    __shared__ StatesStepShared<S, NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // logit[t][S], t < T (a data step's)
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = T >> 3, k = n - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    if (!pilot) MVN_STATES_PHASE1()  // ---- phase 1: the word's tiles, round-robin over the waves
    __syncthreads();
    if (wave != 0) return;
    if (!pilot) {
        // ---- phase 2: wave 0 sweeps the word
        float *decb = dec ? dec + r * dec_ld : nullptr;
        unsigned char *dbits = sh.dbits;
        states_sweep_word<S>(states_logit, T, lane, [&](int t, float mydec) {
            if (decb) decb[t] = mydec;
            dbits[t] = (unsigned char)mydec;
        });
    }
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, C::MEM>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}

// ---- The same step on the TRACED-BACK PATH (mvn_vnet_byword_step_states_path_f32): byword_path_step_kernel's counterpart at these
// state counts.  A data step in the frame above, unchanged (the kernel keeps its own staging lines, as the kernels of
// byword_step.inc do, and expands MVN_STATES_PHASE1 in its own body); what differs is what the lone wave makes of the image.
//   sweep   states_sweep_word's recurrence -- same candidates, same min2_torch_dev -- that also keeps torch.min's index as
//           sweep_surv_kernel defines it: second = !(v1 >= v0) && v0 == v0, v0 the candidate of predecessor 2 s mod S (the first
//           minimum, the first NaN).  States s and s + S / 2 have the same two predecessors, hence the same candidates and the same
//           bit: a stage's survivors are at most 64 distinct bits at every S <= 128, ONE __ballot, and bit (sigma mod 64) of it is
//           state sigma's.  Row t of the image is in the wave's registers when stage t runs (the chunk was fetched eight stages ahead)
//           and nothing reads its logits again: lane 0 puts the stage's ballot into the row's first one or two dwords.  No metric
//           is written back, no running decision is taken, no LDS beyond the running step's: the same longest word.
//   argmin  sigma_T = torch.argmin of the final metrics over the lanes (first minimum, a NaN minimal, the lower index among equals:
//           traceback_kernel's loop as an order on (value, index) pairs; at 128 states the upper half repeats the lower).
//   walk    for t = T - 1 ... 0: j = bit sigma of stage t's survivors, sigma = (2 sigma + j) mod S, bit[t] = sigma & 1
//           (mvn_traceback_f32's bits).  A stage's word sits at an address that does not depend on the path, so 32 stages are ONE
//           load, a stage per lane, requested before the 32 stages above them are walked; the walk takes each word from its lane
//           (readlane) and is scalar arithmetic, every lane alike.  Lane e of each 32 stages stores bit e to dbits and dec.
// The survivor dwords travel through the float image as bit patterns (__uint_as_float: moves, no arithmetic touches them).
// LIST (byword_list_states.inc): the image KEEPS its logits and is only read; a stage's ballot goes to `surv` (one dword per stage, two
// when kWide), the walk fetches it from there, and the metric before stage t goes to the half-image alpha[t][S / 2].  The path form
// takes neither (nullptr).
template <int S, bool LIST = false>
__device__ __forceinline__ void states_path_word(float *image, float *alpha, unsigned *surv, int T, int lane, unsigned char *dbits,
                                                 float *__restrict__ dec) {
    using C = StatesCfg<S>;
    constexpr int LPB = C::LPB, R = C::R, TC = 8, WK = 32, H = S / 2;
    constexpr bool kWide = S > 32;  // the survivors of a stage take two dwords
    constexpr int SW = kWide ? 2 : 1;
    const int sl = lane % LPB;
    const int src0 = (2 * sl) % LPB, src1 = src0 + 1;
    float m = 0.0f;  // (128 states: a lane's two states end every stage with one value)
    auto load_chunk = [&](int t0, float (&c)[TC][R]) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) c[i][r] = image[(t0 + i) * S + sl + LPB * r];
    };
    float cur[TC][R], nxt[TC][R];
    load_chunk(0, nxt);
    for (int t0 = 0; t0 < T; t0 += TC) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) cur[i][r] = nxt[i][r];
        if (t0 + TC < T) load_chunk(t0 + TC, nxt);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            if constexpr (LIST)
                if (lane < H) alpha[(t0 + i) * H + lane] = m;  // the metric before stage t0 + i of states lane and lane + S / 2
            float a[R];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = m + -cur[i][r];
            float v0 = __shfl(a[0], src0), v1 = __shfl(a[0], src1);
            if (R == 2) {
                const float w0 = __shfl(a[R - 1], src0), w1 = __shfl(a[R - 1], src1);
                v0 = sl < 32 ? v0 : w0;
                v1 = sl < 32 ? v1 : w1;
            }
            const bool second = !(v1 >= v0) && v0 == v0;  // torch.min(dim): the first minimal index, the first NaN
            m = min2_torch_dev(v0, v1);
            const unsigned long long bal = __ballot(second);
            if (lane == 0) {
                if constexpr (LIST) {
                    surv[(t0 + i) * SW] = (unsigned)bal;
                    if (kWide) surv[(t0 + i) * SW + SW - 1] = (unsigned)(bal >> 32);
                } else {
                    float *row = image + (t0 + i) * S;
                    row[0] = __uint_as_float((unsigned)bal);
                    if (kWide) row[1] = __uint_as_float((unsigned)(bal >> 32));
                }
            }
        }
    }
    wave_lds_fence();
    int s;
    {
        float bv = m;
        int bi = sl;
#pragma unroll
        for (int off = 1; off < LPB; off <<= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            const bool onan = ov != ov, bnan = bv != bv;
            const bool take = onan ? (!bnan || oi < bi) : (!bnan && ((ov < bv) || (ov == bv && oi < bi)));
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        s = __builtin_amdgcn_readfirstlane(bi);
    }
    // lane l's word of the 32 stages from `base`: stage base + (l & 31); a stage below 0 walks zeros, its bit is not stored
    auto fetch = [&](int base, unsigned &lo, unsigned &hi) {
        const int t = base + (lane & (WK - 1));
        lo = hi = 0u;
        if (t >= 0) {
            if constexpr (LIST) {
                lo = surv[t * SW];
                if (kWide) hi = surv[t * SW + SW - 1];
            } else {
                lo = __float_as_uint(image[t * S]);
                if (kWide) hi = __float_as_uint(image[t * S + 1]);
            }
        }
    };
    unsigned clo, chi, nlo, nhi;
    fetch(T - WK, clo, chi);
    for (int base = T - WK; base > -WK; base -= WK) {
        fetch(base - WK, nlo, nhi);
        unsigned path = 0;  // bit e: symbol base + e
#pragma unroll
        for (int e = WK - 1; e >= 0; --e) {
            unsigned w = (unsigned)__builtin_amdgcn_readlane((int)clo, e);
            if (kWide) {
                const unsigned wh = (unsigned)__builtin_amdgcn_readlane((int)chi, e);
                w = (s & 32) ? wh : w;
            }
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
        clo = nlo;
        chi = nhi;
    }
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_path_step_states_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym) {
    using C = StatesCfg<S>;
    __shared__ StatesStepShared<S, NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // logit[t][S], t < T; then the survivors, a row per stage
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
    MVN_STATES_PHASE1()  // ---- phase 1: the word's tiles, round-robin over the waves
    __syncthreads();
    if (wave != 0) return;
    // ---- phase 2: wave 0 sweeps the word, walks its survivors back and carries on with the codec
    states_path_word<S>(states_logit, nullptr, nullptr, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, C::MEM>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}
