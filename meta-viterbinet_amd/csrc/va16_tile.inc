// va16_tile.inc -- classical Viterbi at 16 states, ONE wave per block (included by mvn_hip.hip after vnet16_fusedn.inc).
//
// The low-latency form of mvn_va_decode_f32 for batches that do not fill the chip (BASELINE configs[0]: 100 blocks x 1000
// symbols).  sweep16_rows_kernel packs four blocks into a wave and takes a decision (a 9-instruction DPP reduction) after
// every trellis step, 214 cycles per step for a wave on its own; here the four 16-lane rows of a wave take turns on the SAME
// block exactly like the sweep of the fused ViterbiNet kernel (row q owns steps 4q..4q+3 of a 16-step tile and hands the
// state vector on with one ds_bpermute), the metrics seen before each step are recorded, and the 16 decisions of a tile are
// taken by four reductions, one per phase, all rows at once: the recurrence's critical path is v_add_f32 + v_min_f32_dpp per
// step and the decisions fill its issue gaps (~30 cycles per step for a lone wave).  Branch costs are the four separately
// rounded operations of va_detector.py:64-68, computed per tile from y and the lane's four state priors.
constexpr int kVaTileWaves = 4;

// One block by the calling wave: emit(t, decision) is called by the lane that holds the decision of symbol t (4 lanes per row and
// 16-step tile); returns the lane's final path metric (meaningful in row 0: logical state logical_state(j, T & 3)).
template <class Emit>
__device__ __forceinline__ float va16_tile_block(const float *__restrict__ yb, const float *__restrict__ prior_row, int T, Emit emit) {
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, q = lane >> 4;
    int ulog[4];
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ulog[r] = logical_state(j, r);
        pr[r] = prior_row[ulog[r]];  // prior of the logical state this lane holds at phase r
    }
    // a non-finite (or absurdly large) state prior makes SOME of a symbol's branch costs NaN: torch.min's NaN rule applies
    // (vnet16_common.inc); wave-uniform, decided once
    const bool strict = __any(needs_strict_min(pr[0]) | needs_strict_min(pr[1]) | needs_strict_min(pr[2]) | needs_strict_min(pr[3]));
    const int row_time = row_time_of(q);  // rows sweep in the order 0, 1, 3, 2
    float m = 0.0f;  // va_detector.py:84

    float ynext[4], prec[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // prec: metrics recorded in the previous tile
#pragma unroll
    for (int r = 0; r < 4; ++r) ynext[r] = yb[row_time + r < T ? row_time + r : T - 1];
    for (int tu = 0; tu < T; tu += 16) {
        const int nsteps = T - tu < 16 ? T - tu : 16;
        float cost[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cost[r] = va_cost(ynext[r], pr[r]);
            const int tn = tu + 16 + row_time + r;
            ynext[r] = yb[tn < T ? tn : T - 1];  // the next tile's samples, requested a tile ahead
        }
        float mrec[4];
        mrec[0] = mrec[1] = mrec[2] = mrec[3] = 0.0f;
        // The decisions of the PREVIOUS tile (four independent DPP reductions over its recorded metrics) are issued between
        // the phases of this tile's sweep: a lone wave issues in order, so they fill the stall slots of the recurrence's
        // dependent add -> min chain instead of following it.
        int d[4] = {0, 0, 0, 0};
        auto sweep_tile = [&](auto full, auto strict_c) {
            constexpr bool F = decltype(full)::value, ST = decltype(strict_c)::value;
            sweep16_tile<F, ST, false>(m, cost, mrec, nsteps, 0, q, [&](auto ph) {
                constexpr int R = decltype(ph)::value;
                d[R] = decide16<R, ST>(prec[R], ulog[R]);
            });
        };
        if (strict) sweep_tile(std::false_type{}, std::true_type{});
        else if (nsteps == 16) sweep_tile(std::true_type{}, std::false_type{});
        else sweep_tile(std::false_type{}, std::false_type{});
        if (tu > 0) {  // emit the previous tile's 16 decisions (a full tile: only the last one can be partial)
            const float mydec = (float)(j == 0 ? d[0] : j == 1 ? d[1] : j == 2 ? d[2] : d[3]);
            if (j < 4) emit(tu - 16 + row_time + j, mydec);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) prec[r] = mrec[r];
    }
    {  // the last tile's decisions
        const int tu = ((T - 1) >> 4) << 4, nsteps = T - tu;
        const float mydec = strict ? decide4<true>(prec, ulog, j) : decide4<false>(prec, ulog, j);
        if (j < 4 && row_time + j < nsteps) emit(tu + row_time + j, mydec);
    }
    return m;
}

// The same sweep keeping the SURVIVORS instead of the running decisions (the by-word step's traced-back decision, byword_step.inc):
// the survivor words of the previous tile (surv16_tile_store, from its recorded metrics + costs) take the decisions' place between
// the phases; afterwards surv_words[0 .. T) hold every step's word and fm[16] the final metric in logical state order (both LDS,
// written and fenced by the calling wave).  Same recurrence, same NaN rule for non-finite priors.
// KEEP (the list step, byword_step.inc): the branch costs and the metrics before every step are left in LDS as well, cost_img[t][state]
// and alpha_img[t][state], 16 * ceil(T / 16) rows each.
template <bool KEEP = false>
__device__ __forceinline__ void va16_tile_block_surv(const float *__restrict__ yb, const float *__restrict__ prior_row, int T,
                                                     unsigned short *surv_words, float *fm, float *cost_img = nullptr,
                                                     float *alpha_img = nullptr) {
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, q = lane >> 4;
    int ulog[4];
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ulog[r] = logical_state(j, r);
        pr[r] = prior_row[ulog[r]];
    }
    const bool strict = __any(needs_strict_min(pr[0]) | needs_strict_min(pr[1]) | needs_strict_min(pr[2]) | needs_strict_min(pr[3]));
    const int row_time = row_time_of(q);
    float m = 0.0f;  // va_detector.py:84

    float ynext[4], pa[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // pa: recorded metric + cost of the previous tile's steps
#pragma unroll
    for (int r = 0; r < 4; ++r) ynext[r] = yb[row_time + r < T ? row_time + r : T - 1];
    for (int tu = 0; tu < T; tu += 16) {
        const int nsteps = T - tu < 16 ? T - tu : 16;
        float cost[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cost[r] = va_cost(ynext[r], pr[r]);
            const int tn = tu + 16 + row_time + r;
            ynext[r] = yb[tn < T ? tn : T - 1];
        }
        float mrec[4];
        mrec[0] = mrec[1] = mrec[2] = mrec[3] = 0.0f;
        auto sweep_tile = [&](auto full, auto strict_c) {
            constexpr bool F = decltype(full)::value, ST = decltype(strict_c)::value;
            sweep16_tile<F, ST, false>(m, cost, mrec, nsteps, 0, q, [&](auto ph) {
                if (decltype(ph)::value == 1 && tu > 0) surv16_tile_store(pa, ulog, lane, surv_words + tu - 16);
            });
        };
        if (strict) sweep_tile(std::false_type{}, std::true_type{});
        else if (nsteps == 16) sweep_tile(std::true_type{}, std::false_type{});
        else sweep_tile(std::false_type{}, std::false_type{});
#pragma unroll
        for (int r = 0; r < 4; ++r) pa[r] = mrec[r] + cost[r];
        if (KEEP) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cost_img[(tu + row_time + r) * 16 + ulog[r]] = cost[r];
                alpha_img[(tu + row_time + r) * 16 + ulog[r]] = mrec[r];
            }
        }
    }
    surv16_tile_store(pa, ulog, lane, surv_words + (((T - 1) >> 4) << 4));
    if (q == 0) fm[logical_state(j, T & 3)] = m;
    wave_lds_fence();
}

// ---- The same detector with the two jobs of a block on different waves (round 5; BASELINE configs[0]: 100 blocks x 1000).
// A lone wave issues in order, one vector instruction per ~4.5 cycles: of the ~180 instructions a 16-step tile costs va16_tile_block,
// 32 are the recurrence (v_add_f32 + v_min_f32_dpp per step) and 100 are the four decision reductions -- the block's 93 cycles per
// step are its instruction count, not its dependent chain.  Here a four-wave workgroup owns the block: wave 0 runs the recurrence
// alone (costs, add + min per step, the row hand-offs: ~80 instructions per tile) and records the metrics every lane saw before
// its four steps in LDS, 1 KB per tile, and a counter of finished tiles; the other three waves take the tiles' decisions in turn as
// the recurrence passes them (vnet16_coop.inc's hand-off) -- they are independent of each other -- with the same reductions on the
// same lanes: the same bits.  T <= 1024 (64 KB of LDS), batches of
// up to two blocks per CU; everything else keeps one wave per block.
constexpr int kVaSplitWaves = 4;
constexpr int kVaSplitMaxT = 1024;
__global__ __launch_bounds__(64 * kVaSplitWaves) void va16_split_kernel(const float *__restrict__ y, int64_t y_ld,
                                                                        const float *__restrict__ priors, int64_t Bp,
                                                                        float *__restrict__ dec, int64_t dec_ld,
                                                                        float *__restrict__ final_metric, int64_t B, int T) {
    constexpr int S = 16;
    extern __shared__ float4 va_split_rec[];  // [tile][lane]: the metrics the lane saw before its four steps of the tile
    __shared__ int s_swept;                   // tiles whose records are complete (wave 0 publishes, the others wait for theirs)
    if (threadIdx.x == 0) s_swept = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = blockIdx.x;
    const int j = lane & 15, q = lane >> 4;
    const float *yb = y + b * y_ld, *prior_row = priors + (b % Bp) * S;
    int ulog[4];
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ulog[r] = logical_state(j, r);
        pr[r] = prior_row[ulog[r]];
    }
    const bool strict = __any(needs_strict_min(pr[0]) | needs_strict_min(pr[1]) | needs_strict_min(pr[2]) | needs_strict_min(pr[3]));
    const int row_time = row_time_of(q);  // rows sweep in the order 0, 1, 3, 2
    const int ntiles = (T + 15) >> 4;
    if (wave == 0) {  // ---- the recurrence
        float m = 0.0f;  // va_detector.py:84
        float ynext[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ynext[r] = yb[row_time + r < T ? row_time + r : T - 1];
        for (int tu = 0; tu < T; tu += 16) {
            const int nsteps = T - tu < 16 ? T - tu : 16;
            float cost[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cost[r] = va_cost(ynext[r], pr[r]);
                const int tn = tu + 16 + row_time + r;
                ynext[r] = yb[tn < T ? tn : T - 1];
            }
            // (the live row keeps its metrics before every step with a v_cndmask; exec-masked ds_writes straight into LDS instead were
            // measured slower: 34 vs 28 us for 100 x 1000)
            float mrec[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (strict) sweep16_tile<false, true, false>(m, cost, mrec, nsteps, 0, q);
            else if (nsteps == 16) sweep16_tile<true, false, false>(m, cost, mrec, nsteps, 0, q);
            else sweep16_tile<false, false, false>(m, cost, mrec, nsteps, 0, q);
            va_split_rec[(tu >> 4) * 64 + lane] = make_float4(mrec[0], mrec[1], mrec[2], mrec[3]);
            __hip_atomic_store(&s_swept, (tu >> 4) + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (final_metric && q == 0) final_metric[b * S + logical_state(j, T & 3)] = m;
        return;
    }
    // ---- the decisions: tile k by wave 1 + k % 3, as soon as the recurrence has passed it (wave 0 always gets there: it waits
    // for nobody)
    float *decb = dec + b * dec_ld;
    for (int tile = wave - 1; tile < ntiles; tile += kVaSplitWaves - 1) {
        while (__hip_atomic_load(&s_swept, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= tile) __builtin_amdgcn_s_sleep(1);
        const float4 p4 = va_split_rec[tile * 64 + lane];
        const float prec[4] = {p4.x, p4.y, p4.z, p4.w};
        const float mydec = strict ? decide4<true>(prec, ulog, j) : decide4<false>(prec, ulog, j);
        if (j < 4 && 16 * tile + row_time + j < T) decb[16 * tile + row_time + j] = mydec;
    }
}

// the split form's range: the block's records fit the LDS, and the batch leaves the CUs room for four waves per block
inline bool va16_split_serves(int64_t B, int T) {
    const int n_cu = current_device_cus();
    return T <= kVaSplitMaxT && B <= (int64_t)2 * (n_cu > 0 ? n_cu : 256);
}

__global__ __launch_bounds__(64 * kVaTileWaves) void va16_tile_kernel(const float *__restrict__ y, int64_t y_ld,
                                                                      const float *__restrict__ priors, int64_t Bp,
                                                                      float *__restrict__ dec, int64_t dec_ld,
                                                                      float *__restrict__ final_metric, int64_t B, int T) {
    constexpr int S = 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = (int64_t)blockIdx.x * kVaTileWaves + wave;
    if (b >= B) return;  // whole wave
    float *decb = dec + b * dec_ld;
    const float m = va16_tile_block(y + b * y_ld, priors + (b % Bp) * S, T, [&](int t, float mydec) { decb[t] = mydec; });
    if (final_metric && (lane >> 4) == 0) final_metric[b * S + logical_state(lane & 15, T & 3)] = m;
}

inline int launch_va16_split(const float *y, int64_t y_ld, const float *priors, int64_t Bp, float *dec, int64_t dec_ld,
                             float *final_metric, int64_t B, int T, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    const size_t lds = (size_t)((T + 15) / 16) * 64 * sizeof(float4);
    if (lds > 64 * 1024) return -1;
    if (ensure_dynamic_lds((const void *)va16_split_kernel, lds)) return -1;  // (the caller then takes one wave per block)
    hipLaunchKernelGGL(va16_split_kernel, dim3((unsigned)B), dim3(64 * kVaSplitWaves), lds, st, y, y_ld, priors, Bp, dec, dec_ld,
                       final_metric, B, T);
    return (int)hipGetLastError();
}

inline int launch_va16_tile(const float *y, int64_t y_ld, const float *priors, int64_t Bp, float *dec, int64_t dec_ld,
                            float *final_metric, int64_t B, int T, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    const int64_t grid = (B + kVaTileWaves - 1) / kVaTileWaves;
    hipLaunchKernelGGL(va16_tile_kernel, dim3((unsigned)grid), dim3(64 * kVaTileWaves), 0, st, y, y_ld, priors, Bp, dec, dec_ld,
                       final_metric, B, T);
    return (int)hipGetLastError();
}
