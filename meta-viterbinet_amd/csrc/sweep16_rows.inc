// sweep16_rows.inc -- 16-state (L=4) trellis sweep, one 16-lane ROW per block, 4 blocks per wave.
// Included by mvn_hip.hip inside its anonymous namespace, after vnet16_common.inc (shares the DPP helpers).
//
// This is the HBM-bound kernel of the path (mvn_acs_sweep_f32 at S=16: 64 B of branch costs read and
// 4 B of decision written per symbol) and, with MODE_VA, the fused classical Viterbi detector
// (costs computed in registers from y and the state priors: 8 B/symbol).
//
//   - lane = physical slot of a state vector; the ACS recurrence runs in place exactly as in
//     vnet16_common.inc (partner masks 1,2,7,8, logical state of a slot rotates with period 4), so a
//     stage is v_add_f32 + v_min_f32_dpp;
//   - each lane loads the branch cost of the LOGICAL state it holds at that step straight from HBM
//     (cost[b][t][logical(p, t%4)]): the 16 lanes of a row still cover one contiguous 64-B line, so
//     loads stay fully coalesced and no cross-lane permute is needed;
//   - kRowsBufs x kRowsDepth steps of costs are kept in flight per lane (a ring of register buffers);
//   - decisions: DPP all-reduce min of the metrics, then of the tying logical indices (first minimal
//     index, torch.argmin); 16 decisions are collected across the row's lanes and stored as one
//     64-B line.
constexpr int kRowsWaves = 4;
constexpr int kRowsDepth = 16;  // steps per chunk (= one 64-B decision line)
#ifndef MVN_ROWS_BUFS
#define MVN_ROWS_BUFS 3
#endif
constexpr int kRowsBufs = MVN_ROWS_BUFS;  // chunks in flight

template <int MODE>
__global__ __launch_bounds__(64 * kRowsWaves) void sweep16_rows_kernel(
    const float *__restrict__ src, int64_t src_ld, const float *__restrict__ priors, int64_t Bp,
    float *__restrict__ dec, int64_t dec_ld, float *__restrict__ final_metric, int64_t B, int T) {
    constexpr int S = 16;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int p = lane & 15;
    const int64_t b = ((int64_t)blockIdx.x * kRowsWaves + wave) * 4 + (lane >> 4);
    const bool active = b < B;
    const int64_t bc = active ? b : B - 1;

    int ulog[4];
    float pr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ulog[r] = logical_state(p, r);
        pr[r] = 0.0f;
        if (MODE == MODE_VA) pr[r] = priors[(bc % Bp) * S + ulog[r]];
    }
    const float *base = (MODE == MODE_VA) ? src + bc * src_ld : src + bc * (int64_t)T * S;

    // raw[i] = input of step t0+i: the cost of this lane's logical state (COST/NEGLOGIT) or y[t] (VA)
    auto load_chunk = [&](int t0, float (&raw)[kRowsDepth]) {
#pragma unroll
        for (int i = 0; i < kRowsDepth; ++i) {
            const int t = t0 + i < T ? t0 + i : T - 1;
            raw[i] = (MODE == MODE_VA) ? base[t] : base[(int64_t)t * S + ulog[i & 3]];
        }
    };

    // kRowsBufs chunks of kRowsDepth steps are in flight per lane (a ring of register buffers): the kernel is
    // HBM-latency bound, so bytes in flight = waves x kRowsBufs x kRowsDepth x 256 B is what sets the rate.
    float buf[kRowsBufs][kRowsDepth], cur[kRowsDepth];
#pragma unroll
    for (int k = 0; k < kRowsBufs; ++k)
        if (k * kRowsDepth < T) load_chunk(k * kRowsDepth, buf[k]);
    float m = 0.0f;  // va_detector.py:84
    bool strict = false;
    for (int tb = 0; tb < T; tb += kRowsDepth * kRowsBufs) {
#pragma unroll
        for (int k = 0; k < kRowsBufs; ++k) {
            const int t0 = tb + k * kRowsDepth;
            if (t0 < T) {  // wave-uniform
#pragma unroll
                for (int i = 0; i < kRowsDepth; ++i) cur[i] = buf[k][i];
                if (t0 + kRowsDepth * kRowsBufs < T) load_chunk(t0 + kRowsDepth * kRowsBufs, buf[k]);
                float mydec = 0.0f;
                if (MODE != MODE_VA && !strict) {  // materialised costs: an odd one (vnet16_common.inc) switches the wave to torch.min's
                    strict = __any(any_odd_cost(cur)) != 0;  // rule for good; the classical Viterbi mode is vouched for by its guard launch
                }
                auto steps = [&](auto strict_c) {
                    constexpr bool ST = decltype(strict_c)::value;
#pragma unroll
                    for (int i = 0; i < kRowsDepth; ++i) {
                        if (t0 + i < T) {  // wave-uniform
                            const int rho = i & 3;  // t0 % 4 == 0
                            // decision from the metrics BEFORE this stage (va_detector.py:93)
                            int bit;
                            if (ST)
                                bit = rho == 0 ? decide_lsb_strict<0>(m, ulog[0]) : rho == 1 ? decide_lsb_strict<1>(m, ulog[1])
                                    : rho == 2 ? decide_lsb_strict<2>(m, ulog[2]) : decide_lsb_strict<3>(m, ulog[3]);
                            else
                                bit = rho == 0 ? decide_lsb<0>(m, ulog[0]) : rho == 1 ? decide_lsb<1>(m, ulog[1])
                                    : rho == 2 ? decide_lsb<2>(m, ulog[2]) : decide_lsb<3>(m, ulog[3]);
                            if (p == i) mydec = (float)bit;
                            float c = cur[i];
                            if (MODE == MODE_VA) c = va_cost(c, pr[rho]);
                            if (MODE == MODE_NEGLOGIT) c = -c;
                            if (ST)
                                m = rho == 0 ? acs_inplace_strict<0>(m, c) : rho == 1 ? acs_inplace_strict<1>(m, c)
                                  : rho == 2 ? acs_inplace_strict<2>(m, c) : acs_inplace_strict<3>(m, c);
                            else
                                m = rho == 0 ? acs_inplace<0>(m, c) : rho == 1 ? acs_inplace<1>(m, c)
                                  : rho == 2 ? acs_inplace<2>(m, c) : acs_inplace<3>(m, c);
                        }
                    }
                };
                if (MODE != MODE_VA && strict) steps(std::true_type{});
                else steps(std::false_type{});
                if (active && t0 + p < T) dec[b * dec_ld + t0 + p] = mydec;
            }
        }
    }
    if (active && final_metric) final_metric[b * S + logical_state(p, T & 3)] = m;
}

template <int MODE>
int launch_sweep16_rows(const float *src, int64_t src_ld, const float *priors, int64_t Bp, float *dec,
                        int64_t dec_ld, float *final_metric, int64_t B, int T, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    constexpr int per_wg = kRowsWaves * 4;
    const int64_t grid = (B + per_wg - 1) / per_wg;
    hipLaunchKernelGGL((sweep16_rows_kernel<MODE>), dim3((unsigned)grid), dim3(64 * kRowsWaves), 0, st, src, src_ld,
                       priors, Bp, dec, dec_ld, final_metric, B, T);
    return (int)hipGetLastError();
}
