// va_inplace.inc -- fused classical Viterbi detector for any S = 4 << LB states (LB = 0..6: S = 4..256), included by
// mvn_hip.hip after va16_quad.inc (shares the DPP helpers and the in-lane minima).
//
// The in-place ACS recurrence of va16_quad.inc (its LB = 2 instance, tuned separately), written once for every split
// of the state index into LB lane bits and 2 register bits: a block's S path metrics live in 2^LB lanes x 4 VGPRs and
// never move; stage t uses the partner operation of phase rho = t % (LB + 2):
//     rho < LB    : lane ^ {1, 2, 7, 8, 16, 32}[rho]   (DPP quad_perm / row_half_mirror / row_ror:8, ds_bpermute)
//     rho = LB    : register ^ 1                        (in-lane)
//     rho = LB + 1: register ^ 2                        (in-lane)
// and the slot with coordinates X (lane bits in the basis above, then the register bits) holds logical state
// rotr(X, rho).  Decisions (va_detector.py:93): before a stage the metrics are equal in the pairs joined by the previous
// stage's operation and those two slots hold logical states s and s + S/2, so reducing over the other operations gives
// the block minimum everywhere and the minimal tying index up to + S/2 -- the same least-significant bit.
// Serves S = 4, 8, 32, 64, 128, 256 (BASELINE configs[3] is S = 256: 1.49e10 symbols/s = 3.8e12 state-steps/s at
// 125 000 blocks x 1000, 7 % above the 256-state-only kernel it replaced); S = 16 keeps va16_quad_kernel (1.4x faster
// there), S = 2 keeps sweep_kernel.  tests/ and tools/fuzz_parity.py cross-check every LB against the oracle.
// A wave owns 64 >> LB blocks.  y and the decisions are staged per wave in LDS, 64 steps at a time (32 at S = 4, to
// stay inside 64 KB of static LDS): coalesced row pieces in and out, the next chunk of y prefetched into registers, one
// broadcast ds_read and one ds_write per step.  That keeps the phase unrolling (LB + 2 steps) independent of the
// staging granularity.
constexpr int kVaIpWaves = 4;

__device__ __forceinline__ float bperm_f32(float v, int byte_addr) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}

template <int LB>
__device__ __forceinline__ int va_ip_coords(int p, int r) {
    int x = p;
    if (LB >= 3) {  // lane ^ 7 must flip one coordinate only: x0 = p0 ^ p2, x1 = p1 ^ p2, x2 = p2
        const int l2 = (p >> 2) & 1;
        x = (p & ~3) | ((p & 1) ^ l2) | ((((p >> 1) & 1) ^ l2) << 1);
    }
    return x | (r << LB);
}

template <int K>
__device__ __forceinline__ float va_ip_lane_min(float v, int lane) {
    if (K == 0) return min_xor1(v);
    if (K == 1) return min_xor2(v);
    if (K == 2) return min_xor7(v);
    if (K == 3) return min_xor8(v);
    return vmin2(v, bperm_f32(v, 4 * (lane ^ (K == 4 ? 16 : 32))));
}
template <int K>
__device__ __forceinline__ int va_ip_lane_imin(int v, int lane) {
    if (K == 0) return min(v, dpp_i32<MVN_DPP_XOR1>(v));
    if (K == 1) return min(v, dpp_i32<MVN_DPP_XOR2>(v));
    if (K == 2) return min(v, dpp_i32<MVN_DPP_XOR7>(v));
    if (K == 3) return min(v, dpp_i32<MVN_DPP_XOR8>(v));
    return min(v, __builtin_amdgcn_ds_bpermute(4 * (lane ^ (K == 4 ? 16 : 32)), v));
}

// LSB of the first minimal logical state before a phase-RHO stage.  As in the other in-place kernels the metrics are
// equal in the pairs joined by the previous stage's operation (logical states s and s + S/2): that operation is skipped.
// (_u: the slots' logical states at this phase are given -- u[r] = bits RHO .. RHO + N - 1 of XX[r] -- e.g. read from a table)
template <int LB, int RHO>
__device__ __forceinline__ int va_ip_decide_u(const float (&m)[4], const int (&u)[4], int lane) {
    constexpr int N = LB + 2, PREV = (RHO + N - 1) % N;
    float v;
    if (PREV == LB) v = vmin2(m[0], m[2]);           // registers r and r^1 are equal
    else if (PREV == LB + 1) v = vmin2(m[0], m[1]);  // registers r and r^2 are equal
    else v = vmin3(m[0], m[1], vmin2(m[2], m[3]));
    if (LB > 0 && PREV != 0) v = va_ip_lane_min<0>(v, lane);
    if (LB > 1 && PREV != 1) v = va_ip_lane_min<1>(v, lane);
    if (LB > 2 && PREV != 2) v = va_ip_lane_min<2>(v, lane);
    if (LB > 3 && PREV != 3) v = va_ip_lane_min<3>(v, lane);
    if (LB > 4 && PREV != 4) v = va_ip_lane_min<4>(v, lane);
    if (LB > 5 && PREV != 5) v = va_ip_lane_min<5>(v, lane);
    // the logical state of (lane, r) grows with r among the registers compared here, so the lane's first minimal slot
    // is found by a select chain from the top (checked for every LB and phase when the layout was designed)
    int c = 4 << LB;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
        if (PREV == LB && (r & 1)) continue;
        if (PREV == LB + 1 && (r & 2)) continue;
        c = m[r] == v ? u[r] : c;
    }
    if (LB > 0 && PREV != 0) c = va_ip_lane_imin<0>(c, lane);
    if (LB > 1 && PREV != 1) c = va_ip_lane_imin<1>(c, lane);
    if (LB > 2 && PREV != 2) c = va_ip_lane_imin<2>(c, lane);
    if (LB > 3 && PREV != 3) c = va_ip_lane_imin<3>(c, lane);
    if (LB > 4 && PREV != 4) c = va_ip_lane_imin<4>(c, lane);
    if (LB > 5 && PREV != 5) c = va_ip_lane_imin<5>(c, lane);
    return c & 1;
}
template <int LB, int RHO>
__device__ __forceinline__ int va_ip_decide(const float (&m)[4], const int (&XX)[4], int lane) {
    int u[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) u[r] = (int)__builtin_amdgcn_ubfe((unsigned)XX[r], RHO, LB + 2);
    return va_ip_decide_u<LB, RHO>(m, u, lane);
}

// the ACS stage of phase RHO on candidates a[r] = m[r] + branch cost: every slot takes the minimum with its partner
template <int LB, int RHO>
__device__ __forceinline__ void va_ip_acs(float (&m)[4], const float (&a)[4], int lane) {
    if (RHO < LB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = va_ip_lane_min<(RHO < LB ? RHO : 0)>(a[r], lane);
    } else if (RHO == LB) {
        m[0] = m[1] = vmin2(a[0], a[1]);
        m[2] = m[3] = vmin2(a[2], a[3]);
    } else {
        m[0] = m[2] = vmin2(a[0], a[2]);
        m[1] = m[3] = vmin2(a[1], a[3]);
    }
}

// ---- torch.min's NaN rule for the in-place family (the fused ViterbiNet kernel of vnet_fused_ip.inc when a weight is non-finite
// or huge; the sweeps over materialised costs from the first cost that is NaN, infinite or huge: sweep_inplace.inc)
__device__ __forceinline__ int va_ip_key(float v) { return strict_key(v); }  // (vnet16_common.inc)

template <int K>
__device__ __forceinline__ float va_ip_lane_partner(float v, int lane) {
    if (K == 0) return dpp_f32<MVN_DPP_XOR1>(v);
    if (K == 1) return dpp_f32<MVN_DPP_XOR2>(v);
    if (K == 2) return dpp_f32<MVN_DPP_XOR7>(v);
    if (K == 3) return dpp_f32<MVN_DPP_XOR8>(v);
    return bperm_f32(v, 4 * (lane ^ (K == 4 ? 16 : 32)));
}
template <int LB, int RHO>
__device__ __forceinline__ void va_ip_acs_strict(float (&m)[4], const float (&a)[4], int lane) {
    if (RHO < LB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = min2_strict(a[r], va_ip_lane_partner<(RHO < LB ? RHO : 0)>(a[r], lane));
    } else if (RHO == LB) {
        m[0] = m[1] = min2_strict(a[0], a[1]);
        m[2] = m[3] = min2_strict(a[2], a[3]);
    } else {
        m[0] = m[2] = min2_strict(a[0], a[2]);
        m[1] = m[3] = min2_strict(a[1], a[3]);
    }
}
// va_ip_decide on the integer keys: the same reductions (the pairs joined by the previous stage still hold equal metrics --
// the strict stage writes one value to both partners), with NaN ordered first
template <int LB, int RHO>
__device__ __forceinline__ int va_ip_decide_strict_u(const float (&m)[4], const int (&u)[4], int lane) {
    constexpr int N = LB + 2, PREV = (RHO + N - 1) % N;
    int k[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) k[r] = va_ip_key(m[r]);
    int v;
    if (PREV == LB) v = min(k[0], k[2]);
    else if (PREV == LB + 1) v = min(k[0], k[1]);
    else v = min(min(k[0], k[1]), min(k[2], k[3]));
    if (LB > 0 && PREV != 0) v = va_ip_lane_imin<0>(v, lane);
    if (LB > 1 && PREV != 1) v = va_ip_lane_imin<1>(v, lane);
    if (LB > 2 && PREV != 2) v = va_ip_lane_imin<2>(v, lane);
    if (LB > 3 && PREV != 3) v = va_ip_lane_imin<3>(v, lane);
    if (LB > 4 && PREV != 4) v = va_ip_lane_imin<4>(v, lane);
    if (LB > 5 && PREV != 5) v = va_ip_lane_imin<5>(v, lane);
    int c = 4 << LB;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
        if (PREV == LB && (r & 1)) continue;
        if (PREV == LB + 1 && (r & 2)) continue;
        c = k[r] == v ? u[r] : c;
    }
    if (LB > 0 && PREV != 0) c = va_ip_lane_imin<0>(c, lane);
    if (LB > 1 && PREV != 1) c = va_ip_lane_imin<1>(c, lane);
    if (LB > 2 && PREV != 2) c = va_ip_lane_imin<2>(c, lane);
    if (LB > 3 && PREV != 3) c = va_ip_lane_imin<3>(c, lane);
    if (LB > 4 && PREV != 4) c = va_ip_lane_imin<4>(c, lane);
    if (LB > 5 && PREV != 5) c = va_ip_lane_imin<5>(c, lane);
    return c & 1;
}
template <int LB, int RHO>
__device__ __forceinline__ int va_ip_decide_strict(const float (&m)[4], const int (&XX)[4], int lane) {
    int u[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) u[r] = (int)__builtin_amdgcn_ubfe((unsigned)XX[r], RHO, LB + 2);
    return va_ip_decide_strict_u<LB, RHO>(m, u, lane);
}

template <int LB, int RHO>
__device__ __forceinline__ void va_ip_stage(float (&m)[4], const float (&pri)[4], float yv, int lane) {
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = m[r] + va_cost(yv, pri[r]);
    va_ip_acs<LB, RHO>(m, a, lane);
}

template <int LB>
__global__ __launch_bounds__(64 * kVaIpWaves) void va_inplace_kernel(const float *__restrict__ y, int64_t y_ld,
                                                                     const float *__restrict__ priors, int64_t Bp,
                                                                     float *__restrict__ dec, int64_t dec_ld,
                                                                     float *__restrict__ final_metric, int64_t B, int T) {
    constexpr int N = LB + 2, NL = 1 << LB, S = 4 << LB, BPW = 64 >> LB;
    constexpr int CY = LB == 0 ? 32 : 64;   // steps staged at a time
    constexpr int NK = BPW * CY / 64;       // staged floats per lane
    // per-block rows padded to odd bank counts: in a step all blocks of a wave touch the same column
    constexpr int YS = CY + 1;              // floats per staged y row
    constexpr int DS = CY + 4;              // bytes per staged decision row (17 or 9 banks)
    __shared__ float ybuf[kVaIpWaves][BPW * YS];
    __shared__ unsigned char dbuf[kVaIpWaves][BPW * DS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int p = lane & (NL - 1);
    const int g = lane >> LB;  // block within the wave
    const int64_t b0 = ((int64_t)blockIdx.x * kVaIpWaves + wave) * BPW;
    if (b0 >= B) return;  // whole wave; the LDS staging below is per wave (no workgroup barrier anywhere)
    const int64_t b = b0 + g;
    const bool active = b < B;
    const int64_t bc = active ? b : B - 1;

    int XX[4];
    float pri[N][4];
    const float *pb = priors + (bc % Bp) * S;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int X = va_ip_coords<LB>(p, r);
        XX[r] = X | (X << N);
#pragma unroll
        for (int rho = 0; rho < N; ++rho) pri[rho][r] = pb[(XX[r] >> rho) & (S - 1)];
    }

    // staging: element k = it * 64 + lane of a chunk is step k % CY of block k / CY (consecutive lanes = consecutive
    // steps of a row: coalesced pieces of CY floats)
    float *yw = ybuf[wave];
    unsigned char *dw = dbuf[wave];
    float ynext[NK];
    // (The three staging helpers are forced inline: at 4 and 8 states -- 32 unrolled row accesses each, several call sites -- the
    // inliner left them as functions, and their by-reference captures then lived in 112 bytes of scratch.  The lane id is made
    // opaque inside them so that their NK row addresses are recomputed once per chunk -- a handful of integer instructions per CY
    // trellis steps -- instead of being hoisted out of the time loop and held in 2 NK register pairs.)
    auto prefetch = [&](int t0) __attribute__((always_inline)) {  // y[b0 + blk][t0 .. t0 + CY) into registers; rows and steps clamped, never used past T
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
#pragma unroll
        for (int it = 0; it < NK; ++it) {
            const int k = it * 64 + lane_o, blk = k / CY, j = k % CY;
            const int64_t bb = b0 + blk < B ? b0 + blk : B - 1;
            const int t = t0 + j < T ? t0 + j : T - 1;
            ynext[it] = y[bb * y_ld + t];
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {  // registers -> LDS (the wave's own buffer: LDS operations of a wave complete in order)
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
#pragma unroll
        for (int it = 0; it < NK; ++it) {
            const int k = it * 64 + lane_o;
            yw[(k / CY) * YS + k % CY] = ynext[it];
        }
    };
    auto flush = [&](int t0) __attribute__((always_inline)) {  // decisions of steps t0 .. t0 + CY (those below T)
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
#pragma unroll
        for (int it = 0; it < NK; ++it) {
            const int k = it * 64 + lane_o, blk = k / CY, j = k % CY;
            if (b0 + blk < B && t0 + j < T) dec[(b0 + blk) * dec_ld + t0 + j] = (float)dw[blk * DS + j];
        }
    };

    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // va_detector.py:84
    prefetch(0);
    for (int tb = 0; tb < T; tb += N) {
        auto step = [&](auto rho_c) {
            constexpr int RHO = decltype(rho_c)::value;
            const int t = tb + RHO;
            if (t < T) {  // wave-uniform
                const int j = t & (CY - 1);
                if (j == 0) {  // chunk boundary: write the finished decisions out, bring the prefetched y in, request more
                    if (t) flush(t - CY);
                    commit();
                    if (t + CY < T) prefetch(t + CY);
                }
                const float yv = yw[g * YS + j];  // broadcast read inside a block
                // decision from the metrics BEFORE this stage (va_detector.py:93)
                const int bit = va_ip_decide<LB, RHO>(m, XX, lane);
                if (p == 0) dw[g * DS + j] = (unsigned char)bit;
                va_ip_stage<LB, RHO>(m, pri[RHO], yv, lane);
            }
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        if constexpr (N > 2) step(std::integral_constant<int, 2>{});
        if constexpr (N > 3) step(std::integral_constant<int, 3>{});
        if constexpr (N > 4) step(std::integral_constant<int, 4>{});
        if constexpr (N > 5) step(std::integral_constant<int, 5>{});
        if constexpr (N > 6) step(std::integral_constant<int, 6>{});
        if constexpr (N > 7) step(std::integral_constant<int, 7>{});
    }
    flush((T - 1) & ~(CY - 1));
    if (active && final_metric) {
        const int rho = T % N;
#pragma unroll
        for (int r = 0; r < 4; ++r) final_metric[b * S + ((XX[r] >> rho) & (S - 1))] = m[r];
    }
}

template <int LB>
int launch_va_inplace_lb(const float *y, int64_t y_ld, const float *priors, int64_t Bp, float *dec, int64_t dec_ld,
                         float *final_metric, int64_t B, int T, hipStream_t st) {
    constexpr int per_wg = kVaIpWaves * (64 >> LB);
    const int64_t grid = (B + per_wg - 1) / per_wg;
    hipLaunchKernelGGL((va_inplace_kernel<LB>), dim3((unsigned)grid), dim3(64 * kVaIpWaves), 0, st, y, y_ld, priors, Bp, dec,
                       dec_ld, final_metric, B, T);
    return (int)hipGetLastError();
}

// S = 4 << LB; returns -1 for an S this family does not cover (S = 2)
inline int launch_va_inplace(const float *y, int64_t y_ld, const float *priors, int64_t Bp, float *dec, int64_t dec_ld,
                             float *final_metric, int64_t B, int T, int S, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    switch (S) {
        case 4: return launch_va_inplace_lb<0>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 8: return launch_va_inplace_lb<1>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 16: return launch_va_inplace_lb<2>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 32: return launch_va_inplace_lb<3>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 64: return launch_va_inplace_lb<4>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 128: return launch_va_inplace_lb<5>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        case 256: return launch_va_inplace_lb<6>(y, y_ld, priors, Bp, dec, dec_ld, final_metric, B, T, st);
        default: return -1;
    }
}
