// vnet16_common.inc -- what the 16-state (L=4) ViterbiNet and Viterbi kernels share, included by mvn_hip.hip inside its
// anonymous namespace before all of them.  No kernel lives here: the first half holds the sigmoid, the DPP helpers, the ACS
// stages and torch.min's NaN rule; the second half (from "the 16-state ViterbiNet unit" on) holds the detector's arithmetic --
// weight image, k-loop, tile pass, sweep, decisions -- ONCE, for vnet16_fusedn.inc, vnet16_dealt.inc and vnet16_coop.inc.
//
//   sigmoid : the fast form of sigmoid_from_neg (bit-identical where it applies).
//   sweep   : each 16-lane row is a full trellis state vector.  The ACS recurrence
//             (trellis_utils.py:16-30) runs IN PLACE: the two predecessors 2s,2s+1 of states s and
//             s+8 sit in lanes that differ in one bit of the lane id, both compute
//             min(a, a[partner]) with ONE v_min_f32_dpp (partner masks 1,2,7,8 = quad_perm,
//             quad_perm, row_half_mirror, row_ror:8), and the logical state of a lane rotates with
//             period 4.
//   decide  : the path metrics seen before each step are recorded; after a 16-symbol tile all 4 rows
//             evaluate argmin (first minimal LOGICAL index, torch.argmin) for 4 symbols at once:
//             DPP all-reduce min of the value, then of the candidate indices.

constexpr float kFastSigmoidBound = 86.0f;  // |z| below this: no exp over/underflow, 1+e < 2^126

// Fast sigmoid, valid for |d| <= 86 (checked per tile): same arithmetic as sigmoid_from_neg with
//  - rint/cvt/ldexp replaced by a magic-number add and a shift that builds the power of two
//    (exact: |q| <= 125 keeps every intermediate normal),
//  - the IEEE division replaced by v_rcp_f32 + one Newton step, which is the correctly rounded
//    reciprocal for EVERY float in [1, 2^126] (exhaustively verified on gfx950, tools/ubench.hip).
__device__ __forceinline__ float sigmoid_from_neg_fast(float d) {
    // magic = 1.5 * 2^23 + 126 (even, so t + magic rounds half-way cases like rintf): the low mantissa bits of t2 hold
    // q + 126, and (bits(t2) << 23) is the float 2^(q-1) (exponent field q + 126; |q| <= 125 keeps it normal)
    const float kMagic = 12583038.0f;
    float t = d * 1.442695040888963407359924681001892137426645954152985934135449406931f;
    float t2 = t + kMagic;
    float qf = t2 - kMagic;  // == rintf(t) for |t| < 2^22
    float s = __builtin_fmaf(qf, -0.693145751953125f, d);
    s = __builtin_fmaf(qf, -1.428606765330187045e-06f, s);
    float u = 0.000198527617612853646278381f;
    u = __builtin_fmaf(u, s, 0.00139304355252534151077271f);
    u = __builtin_fmaf(u, s, 0.00833336077630519866943359f);
    u = __builtin_fmaf(u, s, 0.0416664853692054748535156f);
    u = __builtin_fmaf(u, s, 0.166666671633720397949219f);
    u = __builtin_fmaf(u, s, 0.5f);
    // the reference's u1 = 1 + fma(s*s, u, s), e = u1 * 2^q, x = 1 + e: 2*u1 = fma(v, 2, 2) exactly (scaling by 2 commutes
    // with the rounding) and u1 * 2^q = (2 u1) * 2^(q-1) exactly, so x = fma(2 u1, 2^(q-1), 1) rounds the same sum once
    const float v = __builtin_fmaf(s * s, u, s);
    const float u2 = __builtin_fmaf(v, 2.0f, 2.0f);
    const float p = __uint_as_float(__float_as_uint(t2) << 23);
    float x = __builtin_fmaf(u2, p, 1.0f);
    float r = __builtin_amdgcn_rcpf(x);
    float err = __builtin_fmaf(-x, r, 1.0f);
    return __builtin_fmaf(err, r, r);
}

#define MVN_DPP_XOR1 0xB1   /* quad_perm:[1,0,3,2]  lane ^ 1 */
#define MVN_DPP_XOR2 0x4E   /* quad_perm:[2,3,0,1]  lane ^ 2 */
#define MVN_DPP_XOR7 0x141  /* row_half_mirror      lane ^ 7 */
#define MVN_DPP_XOR15 0x140 /* row_mirror           lane ^ 15 */
#define MVN_DPP_XOR8 0x128  /* row_ror:8            lane ^ 8 */

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
// min(a, a[partner]) in ONE instruction.  hipcc does not pad hazards inside asm: the two wait states a DPP
// read needs after a VALU write of the same VGPR are provided by the leading s_nop 1.
#define MVN_MIN_DPP(NAME, CTRL_STR)                                                                   \
    __device__ __forceinline__ float NAME(float a) {                                                  \
        float r;                                                                                      \
        asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %1 " CTRL_STR " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(a)); \
        return r;                                                                                     \
    }
MVN_MIN_DPP(min_xor1, "quad_perm:[1,0,3,2]")
MVN_MIN_DPP(min_xor2, "quad_perm:[2,3,0,1]")
MVN_MIN_DPP(min_xor7, "row_half_mirror")
MVN_MIN_DPP(min_xor15, "row_mirror")
MVN_MIN_DPP(min_xor8, "row_ror:8")
#undef MVN_MIN_DPP

// min(a, a[partner]) of unsigned integers in one instruction (the candidate indices of the decisions)
#define MVN_MINU_DPP(NAME, CTRL_STR)                                                                  \
    __device__ __forceinline__ int NAME(int a) {                                                      \
        int r;                                                                                        \
        asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 " CTRL_STR " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(a)); \
        return r;                                                                                     \
    }
MVN_MINU_DPP(minu_xor1, "quad_perm:[1,0,3,2]")
MVN_MINU_DPP(minu_xor2, "quad_perm:[2,3,0,1]")
MVN_MINU_DPP(minu_xor7, "row_half_mirror")
MVN_MINU_DPP(minu_xor8, "row_ror:8")
#undef MVN_MINU_DPP

__device__ __forceinline__ float row_min_f32(float v) { return min_xor15(min_xor7(min_xor2(min_xor1(v)))); }
__device__ __forceinline__ int row_min_i32(int v) {
    v = min(v, dpp_i32<MVN_DPP_XOR1>(v));
    v = min(v, dpp_i32<MVN_DPP_XOR2>(v));
    v = min(v, dpp_i32<MVN_DPP_XOR7>(v));
    v = min(v, dpp_i32<MVN_DPP_XOR15>(v));
    return v;
}
// Phase-aware all-reduces for the decisions.  Before stage t (phase RHO = t % 4) the metrics come in equal pairs:
// stage t-1 wrote min(a, a[partner]) to both lanes of every pair joined by its mask e[(RHO+3)%4] (and at t = 0 all
// metrics are 0), and the two lanes of a pair hold logical states s and s+8.  So reducing over the OTHER three
// masks already gives every lane the row minimum, and the minimal tying index of a lane's half equals the row's
// minimal index or that index + 8 -- the same least-significant bit, which is all the decision needs.
template <int RHO>
__device__ __forceinline__ float row_min_f32_phase(float v) {
    if (RHO == 0) return min_xor7(min_xor2(min_xor1(v)));  // partner mask of stage t-1 was 8
    if (RHO == 1) return min_xor8(min_xor7(min_xor2(v)));  // ... was 1
    if (RHO == 2) return min_xor8(min_xor7(min_xor1(v)));  // ... was 2
    return min_xor8(min_xor2(min_xor1(v)));                // ... was 7
}
template <int RHO>
__device__ __forceinline__ int row_min_i32_phase(int v) {
    if (RHO != 1) v = minu_xor1(v);  // candidates are 0..16: unsigned min
    if (RHO != 2) v = minu_xor2(v);
    if (RHO != 3) v = minu_xor7(v);
    if (RHO != 0) v = minu_xor8(v);
    return v;
}
// LSB of the first minimal logical state (torch.argmin(in_prob) % 2) of the metrics seen before a phase-RHO stage
template <int RHO>
__device__ __forceinline__ int decide_lsb(float m, int ulog_rho) {
    const float mn = row_min_f32_phase<RHO>(m);
    const int cand = m == mn ? ulog_rho : 16;
    return row_min_i32_phase<RHO>(cand) & 1;
}

// one in-place ACS stage for phase RHO = t % 4
template <int RHO>
__device__ __forceinline__ float acs_inplace(float m, float cost) {
    float a = m + cost;
    if (RHO == 0) return min_xor1(a);
    if (RHO == 1) return min_xor2(a);
    if (RHO == 2) return min_xor7(a);
    return min_xor8(a);
}

// ---- torch.min's NaN rule (trellis_utils.py:30: torch.min(dim) returns NaN when either candidate is NaN).  v_min_f32 is
// IEEE minNum: it DROPS a NaN that sits in only one of the two candidates.  The two agree unless some but not all of a
// symbol's branch costs are NaN (or +inf meets -inf in a path metric), which needs a non-finite or absurdly large weight /
// state prior: the kernels scan those once in their prologue (weights_need_strict_min) and only then take the forms below
// -- two more VALU instructions per stage and a NaN-first candidate rule in the decisions, never on the default path.
constexpr float kStrictMinBound = 1e14f;  // below this no product or sum of weights, activations and T <= 1e6 costs overflows
__device__ __forceinline__ bool needs_strict_min(float w) { return !(fabsf(w) < kStrictMinBound); }  // NaN, inf or huge

// A MATERIALISED branch cost (mvn_acs_sweep_f32, the logits of the two-kernel ViterbiNet route) from which on a sweep must follow
// torch.min's rule: NaN; infinite (inf - inf = NaN at a later stage); or so large that sums of T <= 10^6 such costs could overflow.
// Every cost passes through registers once on its way into the recurrence: the sweeps test it there (one v_cmp per register, the
// kernels are HBM-bound) and switch to the NaN-propagating stage and decision for the rest of the wave's blocks (sticky: a NaN
// path metric spreads to all states within log2 S stages and stays).
constexpr float kOddCostBound = 1e30f;
__device__ __forceinline__ bool odd_cost(float c) { return !(fabsf(c) < kOddCostBound); }
// The same test for N costs at once at half an instruction per cost: their squares are summed in packed accumulators
// (v_pk_fma_f32, four independent chains) and the sum is compared once.  NaN and inf survive the sum; a cost of 1e18 or more
// overflows it or pushes it past the bound.  The test is one-sided by design: it may also fire for large finite costs that are not
// odd (a wave then merely runs the NaN-propagating forms, which give the same results on such costs); it never misses an odd one.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
constexpr float kOddSquareSumBound = 1e36f;  // sum of squares below this: every |cost| < 1e18 (and finite)
template <int N>
__device__ __forceinline__ bool any_odd_cost(const float (&c)[N]) {
    static_assert(N % 8 == 0, "four packed accumulators");
    f32x2_t acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x2_t{0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < N; i += 8)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x2_t v = {c[i + 2 * k], c[i + 2 * k + 1]};
            acc[k] = __builtin_elementwise_fma(v, v, acc[k]);
        }
    const f32x2_t t = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    return !(t.x + t.y < kOddSquareSumBound);
}
// order-preserving integer image of a path metric with NaN below everything (torch.argmin: the first NaN wins, else the first
// minimum); -0 and +0 compare equal like torch's `<`
__device__ __forceinline__ int strict_key(float v) {
    v += 0.0f;  // -0 -> +0
    const int b = __float_as_int(v);
    return v != v ? (int)0x80000000 : (b < 0 ? b ^ 0x7fffffff : b);
}

template <int RHO>
__device__ __forceinline__ float acs_inplace_strict(float m, float cost) {
    const float a = m + cost;
    const float p = RHO == 0 ? dpp_f32<MVN_DPP_XOR1>(a) : RHO == 1 ? dpp_f32<MVN_DPP_XOR2>(a)
                  : RHO == 2 ? dpp_f32<MVN_DPP_XOR7>(a) : dpp_f32<MVN_DPP_XOR8>(a);
    const float r = fminf(a, p);
    return a != a ? a : (p != p ? p : r);  // both lanes of the pair end up with NaN when either candidate is NaN
}
// torch.argmin(in_prob) % 2 with NaN metrics: the first NaN's index wins; without NaN the first minimum's (decide_lsb).
// The pair argument of decide_lsb holds for NaN-ness too (both lanes of a pair received the same result).
template <int RHO>
__device__ __forceinline__ int decide_lsb_strict(float m, int ulog_rho) {
    const int first_nan = row_min_i32_phase<RHO>(m != m ? ulog_rho : 16);
    const float mn = row_min_f32_phase<RHO>(m);
    const int first_min = row_min_i32_phase<RHO>(m == mn ? ulog_rho : 16);
    return (first_nan < 16 ? first_nan : first_min) & 1;
}

// Logical state held by physical lane p (0..15) of a row at phase rho: lane-id coordinates in the
// basis {1,2,7,8} (x2 = p2, x0 = p0^p2, x1 = p1^p2, x3 = p3), rotated right rho times.
__device__ __forceinline__ int logical_state(int p, int rho) {
    int x[4];
    x[2] = (p >> 2) & 1;
    x[0] = (p & 1) ^ x[2];
    x[1] = ((p >> 1) & 1) ^ x[2];
    x[3] = (p >> 3) & 1;
    int u = 0;
    for (int i = 0; i < 4; ++i) u |= x[(rho + i) & 3] << i;
    return u;
}

// ================================================================================================================================
// The 16-state ViterbiNet unit: the arithmetic of one 16-symbol tile -- the likelihood MLP in the reference's k-ordered fmaf chains,
// the in-place sweep, the decisions -- written ONCE.  vnet16_fusedn_kernel (one wave per block), vnet16_dealt_kernel (32-symbol units
// dealt to rings of waves) and coop_detect_block (a 16-wave workgroup per block: vnet16_coop_kernel and both byword_step_kernel<NS>)
// instantiate it; what differs between them -- tiles in flight, who sweeps, how metrics travel -- stays in their files.  The three
// are each other's cross-check (tests/): a change to the arithmetic or to the NaN rule is made here and reaches all of them.
// ================================================================================================================================

// (wave_lds_fence(), the fence between a wave's LDS writes and its own later reads, is defined at the top of mvn_hip.hip: the
// sweeps included before this file use it too)

// time offset within a tile of row q, and of symbol index i = 4 q + r: the rows sweep in the order 0, 1, 3, 2
constexpr int row_time_of(int q) { return q == 2 ? 12 : q == 3 ? 8 : 4 * q; }
constexpr int sym_time_of(int i) { return row_time_of(i >> 2) + (i & 3); }

// value of lane ((lane + OFF/4) mod 64): ds_bpermute_b32 with the rotation in the instruction's offset field
template <int OFF>
__device__ __forceinline__ float bperm_off(int lane4, float v) {
    float r;
    asm("ds_bpermute_b32 %0, %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(lane4), "v"(v), "n"(OFF));
    return r;
}

// The same hand-off on the vector ALU (v_permlane{16,32}_swap, ~13 cycles of latency instead of an LDS round trip of ~120):
// for the kernels whose sweep is a lone wave's critical path (va16_tile.inc, vnet16_coop.inc); the throughput-bound fused
// kernels use the LDS crossbar form above, which costs the FP32 pipe nothing.  Only the receiving row's copy is used.
template <int K>
__device__ __forceinline__ float row_handoff(float m) {
    const unsigned mu = __float_as_uint(m);
    if (K == 0) return __uint_as_float(__builtin_amdgcn_permlane16_swap(mu, mu, false, false)[0]);  // row 1 <- row 0
    if (K == 1) return __uint_as_float(__builtin_amdgcn_permlane32_swap(mu, mu, false, false)[0]);  // row 3 <- row 1
    if (K == 2) return __uint_as_float(__builtin_amdgcn_permlane16_swap(mu, mu, false, false)[1]);  // row 2 <- row 3
    return __uint_as_float(__builtin_amdgcn_permlane32_swap(mu, mu, false, false)[1]);              // row 0 <- row 2
}

// The workgroup's LDS image of one set of weights, in the layouts the k-loop and the tile pass fetch their operands in.
struct Vnet16Image {
    float ldsB3w[kK3Steps * 64];     // W3 as the layer-3 B operand
    float2 ldsA2xy[kK2Steps * 64];   // (i, lane) -> W2[{0,16} + (lane&15)][4i + (lane>>4)]
    float ldsA2z[kK2Steps * 64];     // (i, lane) -> W2[32 + (lane&15)][4i + (lane>>4)]
    float2 ldsWB[kK2Steps * 4];      // (i, q) -> {-w1, -b1}[4i + q]
    float4 ldsB2[3 * 4];             // (tau, q) -> b2[16 tau + 4 q + {0,1,2,3}]  (D-layout rows of a lane)
    float4 ldsW4849[kK2Steps * 2];   // (i, row) -> W2[48 + row][4i + {0,1,2,3}]
    float ldsMax[2];                 // max |W1|, max |b1|
    float ldsB3[16];                 // b3
    float ldsB2L[2];                 // b2[48], b2[49]

    // Filled by all threads of the workgroup; complete after the caller's barrier.  Every weight passes through here once, so
    // the staging loops also look for the values that make the NaN-propagating ACS minimum necessary ("torch.min's NaN rule"
    // above): returns this thread's part of that answer, for the caller's __syncthreads_or.
    __device__ __forceinline__ bool stage(const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2,
                                          const float *__restrict__ b2, const float *__restrict__ W3, const float *__restrict__ b3) {
        bool odd_w = false;
        for (int e = threadIdx.x; e < kK3Steps * 64; e += blockDim.x) {
            const int l = e & 63, i3 = e >> 6, k = 4 * i3 + (l >> 4);
            const float w3 = k < kH2 ? W3[(l & 15) * kH2 + k] : 0.0f;
            ldsB3w[e] = w3;
            odd_w |= needs_strict_min(w3);
        }
        for (int e = threadIdx.x; e < kK2Steps * 64; e += blockDim.x) {
            const int l = e & 63, i = e >> 6, k = 4 * i + (l >> 4);
            const float wx = W2[(l & 15) * kH1 + k], wy = W2[(16 + (l & 15)) * kH1 + k], wz = W2[(32 + (l & 15)) * kH1 + k];
            ldsA2xy[e] = make_float2(wx, wy);
            ldsA2z[e] = wz;
            odd_w |= needs_strict_min(wx) | needs_strict_min(wy) | needs_strict_min(wz);
        }
        for (int e = threadIdx.x; e < kK2Steps * 4; e += blockDim.x) {
            ldsWB[e] = make_float2(-W1[e], -b1[e]);
            odd_w |= needs_strict_min(W1[e]) | needs_strict_min(b1[e]);
        }
        for (int e = threadIdx.x; e < kK2Steps * 2; e += blockDim.x) {
            const float *wr = W2 + (48 + (e & 1)) * kH1 + 4 * (e >> 1);
            ldsW4849[e] = make_float4(wr[0], wr[1], wr[2], wr[3]);
            odd_w |= needs_strict_min(wr[0]) | needs_strict_min(wr[1]) | needs_strict_min(wr[2]) | needs_strict_min(wr[3]);
        }
        if (threadIdx.x < kH2) odd_w |= needs_strict_min(b2[threadIdx.x]);
        if (threadIdx.x < 12) {
            const int u0 = 16 * (threadIdx.x >> 2) + 4 * (threadIdx.x & 3);
            ldsB2[threadIdx.x] = make_float4(b2[u0], b2[u0 + 1], b2[u0 + 2], b2[u0 + 3]);
        }
        if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0) {  // wave 0: max |W1|, max |b1| over the 100 hidden-1 units: two values per lane, xor-butterfly
            const int lane = threadIdx.x & 63;
            float wm = fmaxf(fabsf(W1[lane]), lane + 64 < kH1 ? fabsf(W1[lane + 64]) : 0.0f);
            float bm = fmaxf(fabsf(b1[lane]), lane + 64 < kH1 ? fabsf(b1[lane + 64]) : 0.0f);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                wm = fmaxf(wm, __shfl_xor(wm, off));
                bm = fmaxf(bm, __shfl_xor(bm, off));
            }
            if (lane == 0) {
                ldsMax[0] = wm;
                ldsMax[1] = bm;
            }
        }
        if (threadIdx.x < 16) {
            ldsB3[threadIdx.x] = b3[threadIdx.x];
            odd_w |= needs_strict_min(b3[threadIdx.x]);
        }
        if (threadIdx.x < 2) ldsB2L[threadIdx.x] = b2[48 + threadIdx.x];
        return odd_w;
    }
};

// per lane: logical state of lane (l & 15) at phases 0..3, for the kernels that keep them out of the VGPRs across the k-loop
// (vnet16_coop.inc recomputes them and does without this 1 KB)
struct Vnet16LaneStates {
    int4 ldsLane[64];
    __device__ __forceinline__ void stage() {
        if (threadIdx.x < 64)
            ldsLane[threadIdx.x] = make_int4(logical_state(threadIdx.x & 15, 0), logical_state(threadIdx.x & 15, 1),
                                             logical_state(threadIdx.x & 15, 2), logical_state(threadIdx.x & 15, 3));
    }
};

// The k-loop: layer 2 of NTL live tiles out of the NT the caller holds accumulators for (a tile that is not live keeps its zeros).
//   hidden-2 units 0..47: per k-step and tile one sigmoid (the caller passes sigmoid_from_neg_fast where it has checked the range,
//     else sigmoid_from_neg: same bits either way) and three
//     v_mfma_f32_16x16x4_f32 with W2 from the image;
//   hidden-2 units 48, 49: the k-step's sigmoids go through the wave's image [symbol][k-phase] (tbw + 64 u: this lane's slot for
//     tile u), the lane reads back the four k's of ITS chain symbol (tbr) ONE k-step later, and a k-ordered chain of four v_fmac_f32
//     (the MFMA's fmaf chain, bit for bit) accumulates ch[0] with row `cunit` of W2[48..49]; NC = 2: a lane carries both units (ch[1]).
// lane_k: the lane id (the callers that count VGPRs pass an opaque copy, so that the addresses derived from it are not kept).
// SCHED: sched_barriers that keep the tiles' sigmoids from interleaving (registers); off where one tile is in flight.
// The sigmoid comes as a lambda written in the kernel's own body, not as a template flag or a functor type of this file: with
// those the optimiser lays the peeled first k-steps out differently and the kernels built for 80 VGPRs spill around the k-loop
// (compare the resource table, profiles/vnet16_shared_unit.txt, after any change here).
template <int NTL, bool SCHED, class Sig, int NT, int NC>
__device__ __forceinline__ void vnet16_kloop(Sig sigmoid, const Vnet16Image &img, const float (&yv)[NT], int lane_k, int cunit, float *tbw,
                                             const float4 *tbr, f32x4 (&acc)[NT][3], float (&ch)[NC]) {
    static_assert(NTL <= NT && (NC == 1 || NC == 2), "live tiles of those allocated; one or two unit chains per lane");
    const int qk = lane_k >> 4;
    const float4 *const wch = &img.ldsW4849[cunit];  // + 2 i (NC = 2: second chain at + 1)
    // one k-step (four k's, in order) of this lane's unit chain(s): tr = the four sigmoids of its symbol
    auto chain_step = [&](const float4 tr, const float4 wa, const float4 wb4) {
        ch[0] = __builtin_fmaf(wa.x, tr.x, ch[0]);
        ch[0] = __builtin_fmaf(wa.y, tr.y, ch[0]);
        ch[0] = __builtin_fmaf(wa.z, tr.z, ch[0]);
        ch[0] = __builtin_fmaf(wa.w, tr.w, ch[0]);
        if constexpr (NC == 2) {
            ch[1] = __builtin_fmaf(wb4.x, tr.x, ch[1]);
            ch[1] = __builtin_fmaf(wb4.y, tr.y, ch[1]);
            ch[1] = __builtin_fmaf(wb4.z, tr.z, ch[1]);
            ch[1] = __builtin_fmaf(wb4.w, tr.w, ch[1]);
        }
    };
    for (int i0 = 0; i0 < kK2Steps; i0 += 5) {
#pragma unroll
        for (int ii = 0; ii < 5; ++ii) {
            const int i = i0 + ii;
            const float2 axy = img.ldsA2xy[i * 64 + lane_k];
            const float az = img.ldsA2z[i * 64 + lane_k];
            const float2 wb = img.ldsWB[i * 4 + qk];
            // the image still holds k-step i-1: request it now, consume it after this k-step's sigmoids (their
            // ds_writes are issued after this read, and a wave's LDS operations execute in order)
            float4 tr = make_float4(0.f, 0.f, 0.f, 0.f), wa = tr, wb4 = tr;
            if (i > 0) {
                tr = *tbr;
                wa = wch[2 * (i - 1)];
                if constexpr (NC == 2) wb4 = wch[2 * (i - 1) + 1];
            }
            wave_lds_fence();
            if constexpr (SCHED) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NTL; ++u) {
                const float h = sigmoid(__builtin_fmaf(yv[u], wb.x, wb.y));
                acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(axy.x, h, acc[u][0], 0, 0, 0);
                acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(axy.y, h, acc[u][1], 0, 0, 0);
                acc[u][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(az, h, acc[u][2], 0, 0, 0);
                tbw[64 * u] = h;
                if constexpr (SCHED) __builtin_amdgcn_sched_barrier(0);  // keep the sigmoids from interleaving (registers)
            }
            if (i > 0) chain_step(tr, wa, wb4);
            wave_lds_fence();
        }
    }
    wave_lds_fence();  // (redundant after the last k-step's own fence; the one-tile caller used to do without it)
    chain_step(*tbr, wch[2 * (kK2Steps - 1)], NC == 2 ? wch[2 * (kK2Steps - 1) + 1] : make_float4(0.f, 0.f, 0.f, 0.f));
}

// Units 48, 49 after the k-loop: bias + ReLU, then back through the image into the layer-3 operand layout: hl[u] = h2[48 + q] of
// symbol (16 u + j) at row q (k-phases 2, 3 of the last operand are zero).  Pointers and cunit as in the k-loop.
template <int NT, int NC>
__device__ __forceinline__ void vnet16_units4849(const Vnet16Image &img, int cunit, const float *tbw, float4 *tbr,
                                                 const float (&ch)[NC], float (&hl)[NT]) {
    wave_lds_fence();
    const float za = ch[0] + img.ldsB2L[cunit];
    const float ra = za < 0.0f ? 0.0f : za;
    if constexpr (NC == 2) {
        const float zb = ch[1] + img.ldsB2L[1];
        *tbr = make_float4(ra, zb < 0.0f ? 0.0f : zb, 0.0f, 0.0f);
    } else {
        float *slot = reinterpret_cast<float *>(tbr) + cunit;
        slot[0] = ra;
        slot[2] = 0.0f;
    }
    wave_lds_fence();
#pragma unroll
    for (int u = 0; u < NT; ++u) hl[u] = tbw[64 * u];
    wave_lds_fence();
}

// The tile pass of NTT tiles together (their layer-3 chains interleave: the phase is latency, not work): bias + ReLU in the MFMA's D
// layout (lane (j,q), register r = unit 16 tau + 4q + r of symbol j), then the (q,r) transpose that puts k in natural order for
// layer 3 -- through the wave's LDS image, rows of 20 dwords per symbol and one image of 80 float4 per tile (one ds_write_b128 and
// four conflict-free ds_read_b32 per row tile) instead of four v_permlane*_swap: LDS instructions cost the SIMD's FP32 pipe nothing,
// a swap costs it 13 cycles here -- and the 13 layer-3 MFMAs.  logit[u][r]: state j at time row_time_of(q) + r of tile u.
template <int NTT>
__device__ __forceinline__ void vnet16_tile_pass(const Vnet16Image &img, float4 *tbase, int lane_t, const f32x4 (*acc)[3],
                                                 const float *hl, float (*logit)[4]) {
    const int jt = lane_t & 15, qt = lane_t >> 4;
    float4 *const ttw = tbase + 5 * jt + qt;                                        // + 80 u: row j, units 4q..4q+3
    const float *const ttr = reinterpret_cast<const float *>(tbase + 5 * jt) + qt;  // + 320 u + 4 r': unit 4r' + q of row j
    float bop[NTT][13];
#pragma unroll
    for (int tau = 0; tau < 3; ++tau) {
        const float4 bb = img.ldsB2[tau * 4 + qt];
        const float bbr[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
        for (int u = 0; u < NTT; ++u) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = acc[u][tau][r] + bbr[r];
                v[r] = z < 0.0f ? 0.0f : z;  // relu; NaN propagates like torch's
            }
            ttw[80 * u] = make_float4(v[0], v[1], v[2], v[3]);
        }
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < NTT; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) bop[u][4 * tau + r] = ttr[320 * u + 4 * r];
        wave_lds_fence();
    }
    f32x4 acc3[NTT];
#pragma unroll
    for (int u = 0; u < NTT; ++u) {
        bop[u][12] = hl[u];
        acc3[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i3 = 0; i3 < kK3Steps; ++i3) {
        const float w3 = img.ldsB3w[i3 * 64 + lane_t];
#pragma unroll
        for (int u = 0; u < NTT; ++u) acc3[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(bop[u][i3], w3, acc3[u], 0, 0, 0);
    }
    const float b3s = img.ldsB3[jt];
#pragma unroll
    for (int u = 0; u < NTT; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) logit[u][r] = acc3[u][r] + b3s;
}

// Four steps of the in-place recurrence by the row that holds the state vector at phase PH of a tile; the row that is LIVE in this
// phase records the metrics seen before each step (what the decisions are made of).
template <int PH, bool FULL, bool STRICT>
__device__ __forceinline__ void sweep16_phase(float &m, const float (&cost)[4], float (&rec)[4], int nsteps, bool live) {
    auto step = [&](auto r_c) {
        constexpr int R = decltype(r_c)::value;
        if (FULL || 4 * PH + R < nsteps) {
            if (live) rec[R] = m;
            m = STRICT ? acs_inplace_strict<R>(m, cost[R]) : acs_inplace<R>(m, cost[R]);
        }
    };
    step(std::integral_constant<int, 0>{});
    step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 3>{});
}

struct Sweep16NoHook {
    template <class PH>
    __device__ __forceinline__ void operator()(PH) const {}
};

// The sweep of one 16-symbol tile (nsteps of them live; FULL: nsteps == 16 known): m = the wave's state vector, cost[r] = the branch
// cost of the lane's logical state at phase r of ITS row's four steps, rec[r] = the metrics before those steps, q = the lane's row.
// A row hands the state vector to the next one (order 0, 1, 3, 2; only the receiving row's copy is used) through the LDS crossbar
// (XBAR, lane4 = 4 * lane: no memory and no FP32-pipe time) or with v_permlane*_swap (a lone sweeping wave: latency).
// between(integral_constant<PH>) runs after each row's steps, before its hand-off (va16_tile.inc puts independent work there).
template <bool FULL, bool STRICT, bool XBAR, class Hook = Sweep16NoHook>
__device__ __forceinline__ void sweep16_tile(float &m, const float (&cost)[4], float (&rec)[4], int nsteps, int lane4, int q,
                                             Hook between = Hook{}) {
    sweep16_phase<0, FULL, STRICT>(m, cost, rec, nsteps, q == 0);
    between(std::integral_constant<int, 0>{});
    m = XBAR ? bperm_off<192>(lane4, m) : row_handoff<0>(m);  // row 1 <- row 0 (lane - 16)
    sweep16_phase<1, FULL, STRICT>(m, cost, rec, nsteps, q == 1);
    between(std::integral_constant<int, 1>{});
    m = XBAR ? bperm_off<128>(lane4, m) : row_handoff<1>(m);  // row 3 <- row 1 (lane - 32)
    sweep16_phase<2, FULL, STRICT>(m, cost, rec, nsteps, q == 3);
    between(std::integral_constant<int, 2>{});
    m = XBAR ? bperm_off<64>(lane4, m) : row_handoff<2>(m);   // row 2 <- row 3 (lane + 16)
    sweep16_phase<3, FULL, STRICT>(m, cost, rec, nsteps, q == 2);
    between(std::integral_constant<int, 3>{});
    m = XBAR ? bperm_off<128>(lane4, m) : row_handoff<3>(m);  // row 0 <- row 2 (lane + 32)
}

// LSB of the first minimal logical state of the metrics recorded before step R (STRICT: torch.argmin's NaN rule)
template <int R, bool STRICT>
__device__ __forceinline__ int decide16(float rec, int ulog) {
    if constexpr (STRICT) return decide_lsb_strict<R>(rec, ulog);
    else return decide_lsb<R>(rec, ulog);
}
// the decisions of a row's four steps from the metrics it recorded: lane jt < 4 of the row gets the one of step jt
template <bool STRICT>
__device__ __forceinline__ float decide4(const float (&rec)[4], const int (&ulog)[4], int jt) {
    const int d0 = decide16<0, STRICT>(rec[0], ulog[0]), d1 = decide16<1, STRICT>(rec[1], ulog[1]);
    const int d2 = decide16<2, STRICT>(rec[2], ulog[2]), d3 = decide16<3, STRICT>(rec[3], ulog[3]);
    return (float)(jt == 0 ? d0 : jt == 1 ? d1 : jt == 2 ? d2 : d3);
}

// ---- Survivors of the in-place sweep and the walk back along them (the by-word step's traced-back decision, byword_step.inc).
// The step at phase RHO leaves min(a, a[partner]) in both lanes of a pair, a = metric before the step + branch cost; the pair's
// logical states before the step are 2 s and 2 s + 1, the predecessors (j = 0, 1) of the states s and s + 8 it holds afterwards.
// torch.min's index (acs_block's argmin_j, what mvn_*_decode_surv_f32 stores) is j = 1 iff a[2 s + 1] < a[2 s], or a[2 s + 1] is NaN
// and a[2 s] is not.  Kept here per PHYSICAL lane: did the lane's new metric come from its partner?  Exact in either form of the
// sweep (the recorded metrics are the oracle's) and off its chain: one add, one DPP move and two compares per step.
template <int RHO>
__device__ __forceinline__ bool surv_from_partner(float a, int ulog_rho) {
    const float ap = RHO == 0 ? dpp_f32<MVN_DPP_XOR1>(a) : RHO == 1 ? dpp_f32<MVN_DPP_XOR2>(a)
                   : RHO == 2 ? dpp_f32<MVN_DPP_XOR7>(a) : dpp_f32<MVN_DPP_XOR8>(a);
    const bool odd_wins = !((ulog_rho & 1 ? a : ap) >= (ulog_rho & 1 ? ap : a)) && (ulog_rho & 1 ? ap == ap : a == a);
    return (ulog_rho & 1) != 0 ? !odd_wins : odd_wins;
}
// The survivor words of one 16-step tile from a[r] = rec[r] + cost[r] of sweep16_tile (all 64 lanes): word[t] bit p = lane p of the
// row that swept step t took its partner's candidate.  Lane q < 4 stores the four words of row q's steps, tile_words[row_time_of(q) ..].
__device__ __forceinline__ void surv16_tile_store(const float (&a)[4], const int (&ulog)[4], int lane, unsigned short *tile_words) {
    const unsigned long long b0 = __ballot(surv_from_partner<0>(a[0], ulog[0])), b1 = __ballot(surv_from_partner<1>(a[1], ulog[1]));
    const unsigned long long b2 = __ballot(surv_from_partner<2>(a[2], ulog[2])), b3 = __ballot(surv_from_partner<3>(a[3], ulog[3]));
    if (lane < 4) {
        const int sh = 16 * lane;
        const unsigned lo = (unsigned)((b0 >> sh) & 0xffffu) | ((unsigned)((b1 >> sh) & 0xffffu) << 16);
        const unsigned hi = (unsigned)((b2 >> sh) & 0xffffu) | ((unsigned)((b3 >> sh) & 0xffffu) << 16);
        *reinterpret_cast<uint2 *>(tile_words + row_time_of(lane)) = make_uint2(lo, hi);
    }
}
// The walk, by every lane of ONE wave alike (uniform addresses: LDS broadcasts): from the first minimal final metric (torch.argmin, a
// NaN counting as minimal; fm[] in logical order) back along words[0 .. T), T % 8 == 0, eight steps per 16-byte fetch and the fetches
// of the next 32 steps requested before the walk of these; the lane that holds the path's state before step t is
// p_t = p_{t+1} ^ (word[t] bit p_{t+1} ? partner mask of phase t % 4 : 0), and bits[t] = sigma_t & 1 = coordinate t % 4 of p_t in
// logical_state's basis.  Lane e of each 32 steps stores bit e: dbits (LDS, one byte per symbol) and dec (may be null).
__device__ __forceinline__ void path16_walk(const unsigned short *words, const float *fm, int T, int lane, unsigned char *dbits,
                                            float *__restrict__ dec) {
    int s = 0;
    float mv = fm[0];
    if (mv == mv) {
        for (int k = 1; k < 16; ++k) {
            const float x = fm[k];
            if (!(x >= mv)) {
                mv = x;
                s = k;
                if (x != x) break;
            }
        }
    }
    int p = __builtin_ctzll(__ballot(lane < 16 && logical_state(lane, T & 3) == s));
    const uint4 *pieces = reinterpret_cast<const uint4 *>(words);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4 cur[4], nxt[4];
    int top = (T >> 3) - 1;  // the piece of the last eight steps
#pragma unroll
    for (int k = 0; k < 4; ++k) cur[k] = top - k >= 0 ? pieces[top - k] : zero;
    for (; top >= 0; top -= 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) nxt[k] = top - 4 - k >= 0 ? pieces[top - 4 - k] : zero;
        unsigned path = 0;  // bit 8 (3 - k) + e: symbol 8 (top - k) + e
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned dw[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
#pragma unroll
            for (int e = 7; e >= 0; --e) {
                const unsigned w = dw[e >> 1] >> (16 * (e & 1));
                const int mask = (e & 3) == 0 ? 1 : (e & 3) == 1 ? 2 : (e & 3) == 2 ? 7 : 8;
                p ^= ((w >> p) & 1u) ? mask : 0;
                const int bit = (e & 3) == 0 ? (p ^ (p >> 2)) & 1 : (e & 3) == 1 ? ((p >> 1) ^ (p >> 2)) & 1 : (p >> ((e & 3))) & 1;
                path |= (unsigned)bit << (8 * (3 - k) + e);
            }
        }
        const int t = 8 * (top - 3) + lane;  // (pieces below 0 walked zeros: their bits are not stored)
        if (lane < 32 && t >= 0) {
            const int bit = (path >> lane) & 1;
            dbits[t] = (unsigned char)bit;
            if (dec) dec[t] = (float)bit;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
    }
}
