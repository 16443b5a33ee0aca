// sweep16_lds.inc -- HBM-streaming variant of the 16-state row sweep (mvn_acs_sweep_f32 / the sweep of the
// two-kernel ViterbiNet route), included by mvn_hip.hip after sweep16_rows.inc.
//
// sweep16_rows_kernel reads the costs with one dword per lane and step: HBM then sees ~10^4 interleaved streams
// advancing 64 B at a time, and the measured rate saturates at ~4.4 TB/s however deep the register prefetch is.
// Here each wave moves WHOLE 1-KB pieces (16 steps of one block's [T][16] cost rows, contiguous in HBM) with one
// `global_load_lds_dwordx4` (LDS-DMA: 64 lanes x 16 B, no VGPR staging) into a per-wave LDS ring, kRing chunks
// ahead, and the lanes pick their logical state's cost out of LDS with one ds_read_b32 per step.
//   LDS per wave: kRing x 4 rows x (1 KB + 64 B pad);  per workgroup (4 waves): kRing x 17 KB.
// vmcnt bookkeeping (LDS-DMA, loads and stores count together, in issue order): per chunk a wave issues
// 4 DMA pieces (G) and later one decision store (S); when chunk c is consumed the operations younger than G(c) are
// S(c-kRing), then (kRing-1) x {G,S}  ->  s_waitcnt vmcnt(1 + 5*(kRing-1)) in steady state, fewer in the first
// kRing chunks (no stores yet) and vmcnt(0) once prefetching has stopped.
#ifndef MVN_SWEEP_GLDS_AUX
#define MVN_SWEEP_GLDS_AUX 2  /* nt: every cost byte is read once; +11 % at 10 000 blocks, +1 % at 100 000 vs default policy */
#endif
constexpr int kLdsWaves = 4;  // waves per workgroup (independent).  Single-wave workgroups were tried: +5 % at 10 000
                              // blocks, -20 % at 12 000, -7 % at 100 000 (tools/time_sweep.py); not worth a size rule.
constexpr int kLdsRing = 3;
constexpr int kLdsRowFloats = 16 * 16 + 16;  // 16 steps x 16 states + pad (rows land on different banks)
constexpr int kLdsChunkFloats = 4 * kLdsRowFloats;

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int MODE>
__global__ __launch_bounds__(64 * kLdsWaves) void sweep16_lds_kernel(const float *__restrict__ src,
                                                                      float *__restrict__ dec, int64_t dec_ld,
                                                                      float *__restrict__ final_metric, int64_t B, int T) {
    constexpr int S = 16;
    __shared__ float lds[kLdsWaves][kLdsRing][kLdsChunkFloats];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int p = lane & 15;
    const int q = lane >> 4;
    const int64_t b0 = ((int64_t)blockIdx.x * kLdsWaves + wave) * 4;  // first of this wave's 4 blocks
    if (b0 >= B) return;  // whole wave
    const int64_t b = b0 + q;
    const bool active = b < B;

    int ulog[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ulog[r] = logical_state(p, r);

    const int nchunks = (T + 15) / 16;
    // DMA piece of this lane for row r of a chunk: 16 B = states 4*(lane&3).. of step (lane>>2)
    auto issue_chunk = [&](int c, int slot) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int64_t br = b0 + r < B ? b0 + r : B - 1;
            int step = 16 * c + (lane >> 2);
            if (step >= T) step = T - 1;  // partial last chunk: re-read valid data, never used
            const float *g = src + (br * (int64_t)T + step) * S + 4 * (lane & 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                             (__attribute__((address_space(3))) void *)&lds[wave][slot][r * kLdsRowFloats],
                                             16, 0, MVN_SWEEP_GLDS_AUX);
        }
    };

    float m = 0.0f;
    float cur[16];
    auto consume_chunk = [&](int c, int slot) {
        const float *row = &lds[wave][slot][q * kLdsRowFloats];
#pragma unroll
        for (int i = 0; i < 16; ++i) cur[i] = row[i * 16 + ulog[i & 3]];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot may be refilled from here on
    };
    // full = all 16 steps of the chunk exist: no per-step branches, so the scheduler can overlap the (independent)
    // decision chains with the recurrence of the following steps
    bool strict = false;  // wave-uniform, sticky: an odd cost (NaN, infinite, huge: odd_cost(), vnet16_common.inc) has come by
    auto process_chunk = [&](int c, auto full, auto strict_c) {
        constexpr bool ST = decltype(strict_c)::value;
        const int t0 = 16 * c;
        float mydec = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (decltype(full)::value || t0 + i < T) {  // wave-uniform
                const int rho = i & 3;
                int bit;
                if (ST)
                    bit = rho == 0 ? decide_lsb_strict<0>(m, ulog[0]) : rho == 1 ? decide_lsb_strict<1>(m, ulog[1])
                        : rho == 2 ? decide_lsb_strict<2>(m, ulog[2]) : decide_lsb_strict<3>(m, ulog[3]);
                else
                    bit = rho == 0 ? decide_lsb<0>(m, ulog[0]) : rho == 1 ? decide_lsb<1>(m, ulog[1])
                        : rho == 2 ? decide_lsb<2>(m, ulog[2]) : decide_lsb<3>(m, ulog[3]);
                if (p == i) mydec = (float)bit;
                float cc = cur[i];
                if (MODE == MODE_NEGLOGIT) cc = -cc;
                if (ST)
                    m = rho == 0 ? acs_inplace_strict<0>(m, cc) : rho == 1 ? acs_inplace_strict<1>(m, cc)
                      : rho == 2 ? acs_inplace_strict<2>(m, cc) : acs_inplace_strict<3>(m, cc);
                else
                    m = rho == 0 ? acs_inplace<0>(m, cc) : rho == 1 ? acs_inplace<1>(m, cc)
                      : rho == 2 ? acs_inplace<2>(m, cc) : acs_inplace<3>(m, cc);
            }
        }
        if (active && t0 + p < T) dec[b * dec_ld + t0 + p] = mydec;
    };

    // prologue: fill the ring
#pragma unroll
    for (int k = 0; k < kLdsRing; ++k)
        if (k < nchunks) issue_chunk(k, k);

    for (int cb = 0; cb < nchunks; cb += kLdsRing) {
#pragma unroll
        for (int k = 0; k < kLdsRing; ++k) {
            const int c = cb + k;
            if (c < nchunks) {  // wave-uniform
                const bool more = c + kLdsRing < nchunks;
                if (!more || strict) {
                    wait_vmcnt<0>();  // draining: nothing younger is guaranteed to be in flight
                } else if (cb == 0) {
                    // first pass over the ring: younger ops = remaining prologue pieces + {G,S} of earlier chunks
                    if (k == 0) wait_vmcnt<4 * (kLdsRing - 1)>();
                    else if (k == 1) wait_vmcnt<4 * (kLdsRing - 1) + 1>();
                    else wait_vmcnt<4 * (kLdsRing - 1) + 2>();
                } else {
                    wait_vmcnt<1 + 5 * (kLdsRing - 1)>();
                }
                consume_chunk(c, k);
                if (more) issue_chunk(c + kLdsRing, k);
                // (the oddness test runs beside the recurrence on whole chunks; see sweep16_quad.inc)
                if (strict) {
                    process_chunk(c, std::false_type{}, std::true_type{});
                } else if (16 * c + 16 <= T) {
                    const float m0 = m;
                    const bool odd = any_odd_cost(cur);
                    process_chunk(c, std::true_type{}, std::false_type{});
                    if (__any(odd)) {
                        strict = true;
                        m = m0;
                        wait_vmcnt<0>();
                        process_chunk(c, std::false_type{}, std::true_type{});
                    }
                } else {
                    strict = __any(any_odd_cost(cur)) != 0;
                    if (strict) process_chunk(c, std::false_type{}, std::true_type{});
                    else process_chunk(c, std::false_type{}, std::false_type{});
                }
            }
        }
    }
    if (active && final_metric) final_metric[b * S + logical_state(p, T & 3)] = m;
}

template <int MODE>
int launch_sweep16_lds(const float *src, float *dec, int64_t dec_ld, float *final_metric, int64_t B, int T,
                       hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    constexpr int per_wg = kLdsWaves * 4;
    const int64_t grid = (B + per_wg - 1) / per_wg;
    hipLaunchKernelGGL((sweep16_lds_kernel<MODE>), dim3((unsigned)grid), dim3(64 * kLdsWaves), 0, st, src, dec, dec_ld,
                       final_metric, B, T);
    return (int)hipGetLastError();
}
