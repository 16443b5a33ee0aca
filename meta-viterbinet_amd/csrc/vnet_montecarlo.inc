// vnet_montecarlo.inc -- the uncoded Monte-Carlo point of the 16-state ViterbiNet in ONE launch, included by mvn_hip.hip after
// word_gen.inc, va_montecarlo.inc (mc_add_counters) and vnet16_fusedn.inc (SURVEY 8f#1: "fused into the decode kernel so y never
// touches HBM", which va_montecarlo.inc did for the classical detector only).
//
// Trainer.single_eval_at_point (python_code/trainers/trainer.py:222-241) for the detector the project is about: every wave generates
// its word's samples where it consumes them -- generate_quad (word_gen.inc): the same pure function of (seed, word, position) as
// mvn_generate_words_f32 -- runs vnet16_fusedn_kernel<false, 2>'s detector on them and compares the decisions with the bits it
// generated.  The launch reads the taps and the weights and adds to four counters; they equal those of mvn_generate_words_f32 ->
// mvn_vnet_decode_count_f32 on the same seed, bit for bit (tests/test_gpu_vnet_montecarlo.py).
//
// What is the fused detector's stays as it is there (one wave per word, 8 waves per workgroup around one weight image, NT = 2,
// the wave priorities, vnet16_common.inc's arithmetic including the strict form); what this file adds:
//   * the samples come from a wave-private LDS image of kMcRefill = 256 symbols: every 8th super-tile each of the 64 lanes runs ONE
//     generate_quad (no lane repeats another's work) and stores its four samples and its four transmitted bits (a 4-bit mask).  The
//     generator's temporaries -- Philox state, the float64 accumulators, Box-Muller -- live between two super-tiles, where nothing
//     but the path metric is held, and are dead during the k-loop, which is built for 80 VGPRs;
//   * the super-tiles read their 32 samples, and the deciding lanes their transmitted bit, from that image: LDS instructions cost
//     the FP32 pipe nothing;
//   * rounds (launch_vnet_montecarlo): a call enqueues n_rounds launches of B words each, round r on words word0 + r B ...; with a stop
//     rule a one-thread gate kernel between two rounds compares the frame errors counted SO FAR with the target and writes the flag
//     that the next round's waves read.  In-order execution on the stream does the rest: no wave reads a counter that its own round
//     is adding to, nothing spins, a round runs whole or not at all, and the host is not asked.
constexpr int kMcRefill = 256;  // symbols per refill: one generate_quad per lane

// progress[0] = rounds that ran, progress[1] = "skip the next round".  One thread, between two rounds on the same stream.
// F <= 0: no stop rule, the gate only counts.
__global__ __launch_bounds__(64) void vnet_mc_gate_kernel(const unsigned long long *__restrict__ counters, int *__restrict__ progress,
                                                          long long F) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int stop = F > 0 && counters[2] >= (unsigned long long)F;
    progress[1] = stop;
    if (!stop) progress[0] += 1;
}

__global__ __launch_bounds__(64 * kFusedNWaves, FusedNCfg<2>::kMinWgPerCu) void vnet16_mc_kernel(
    const double *__restrict__ h, int64_t Bh, double sigma, uint32_t seed_lo, uint32_t seed_hi, int64_t word0,
    const float *__restrict__ W1, const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2,
    const float *__restrict__ W3, const float *__restrict__ b3, unsigned long long *__restrict__ counters,
    const int *__restrict__ progress, int64_t B, int T) {
    constexpr int NT = 2, L = 4;
    constexpr int kSym = 16 * NT;                     // symbols per super-tile
    static_assert(kMcRefill == 4 * 64 && kMcRefill % kSym == 0, "one quad per lane; whole super-tiles per refill");
    __shared__ Vnet16Image img;                       // the weights (vnet16_common.inc)
    __shared__ float4 ldsT[kFusedNWaves][80];         // wave-private scratch image of the k-loop and the tile pass (vnet16_fusedn.inc)
    __shared__ Vnet16LaneStates lanes;
    __shared__ float4 ldsY[kFusedNWaves][64];         // wave-private: the refill's samples, quad by quad
    __shared__ unsigned ldsTx[kFusedNWaves][64];      // ... and the quads' transmitted bits (bit i = symbol 4 quad + i)

    if (progress && progress[1]) return;  // the gate closed this round (uniform over the launch: before any barrier)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row pointers stay in SGPRs

    const bool odd_w = img.stage(W1, b1, W2, b2, W3, b3);
    lanes.stage();
    const bool strict = __syncthreads_or(odd_w) != 0;  // the prologue's barrier; workgroup-uniform
    const float wmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[0])));
    const float bmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[1])));

    const int64_t bl = (int64_t)blockIdx.x * kFusedNWaves + wave;
    if (bl >= B) return;  // whole wave; no barriers below
    const int64_t b = word0 + bl;  // the word's place in the generator's sequence
    // (the 64-bit remainder comes out of the vector ALU.  The row is wave-uniform, which the compiler knows -- it drops a
    // readfirstlane builtin and keeps the taps' address in a VGPR pair across the k-loop: the asm puts it into scalar registers)
    const int64_t hrow = b % Bh;
    unsigned hrow_lo, hrow_hi;
    asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(hrow_lo) : "v"((unsigned)hrow));
    asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(hrow_hi) : "v"((unsigned)(hrow >> 32)));
    const double *const hb = h + (int64_t)(((uint64_t)hrow_hi << 32) | hrow_lo) * L;

    float4 *const tbase = &ldsT[wave][0];
    const float *const ybase = reinterpret_cast<const float *>(&ldsY[wave][0]);
    int nerr = 0;
    float m = 0.0f;

    const int third = (T + 2) / 3;
    for (int t0 = 0; t0 < T; t0 += kSym) {
        const int s0 = t0 & ~(kMcRefill - 1);  // first symbol of the image
        if (t0 == s0) {  // refill (wave-uniform): lane l generates symbols s0 + 4 l .. s0 + 4 l + 3
            int lane_g = lane;
            asm volatile("" : "+v"(lane_g));
            float gy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            unsigned gtx = 0;
            if (s0 + 4 * lane_g < T) generate_quad(seed_lo, seed_hi, b, s0 + 4 * lane_g, T, L, hb, sigma, gy, gtx);
            ldsY[wave][lane_g] = make_float4(gy[0], gy[1], gy[2], gy[3]);
            ldsTx[wave][lane_g] = gtx;
            wave_lds_fence();
        }
#if MVN_FN_PRIO
        if (t0 < third) __builtin_amdgcn_s_setprio(2);
        else if (t0 < 2 * third) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
#endif
        // (per-lane addresses from opaque copies of the lane id, once per phase: see vnet16_fusedn.inc)
        int lane_k = lane;
        asm volatile("" : "+v"(lane_k));
        const int qk = lane_k >> 4;
        float *const tbw = reinterpret_cast<float *>(tbase) + 4 * (lane_k & 15) + qk;
        float4 *const tbr = tbase + (lane_k & 31);
        const int cunit = lane_k >> 5;
        float yv[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int t = t0 + 16 * u + sym_time_of(lane_k & 15);
            yv[u] = ybase[(t < T ? t : T - 1) - s0];  // past the word: its last sample, like the detector that reads y
        }
        float ymax = fabsf(yv[0]);
#pragma unroll
        for (int u = 1; u < NT; ++u) ymax = fmaxf(ymax, fabsf(yv[u]));
        const bool fast = __all(ymax * wmax + bmax <= kFastSigmoidBound);

        f32x4 acc[NT][3];
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int tau = 0; tau < 3; ++tau) acc[u][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ch[1] = {};
        auto kloop = [&](auto sig) { vnet16_kloop<NT, true>(sig, img, yv, lane_k, cunit, tbw, tbr, acc, ch); };
        if (fast) kloop([](float d) { return sigmoid_from_neg_fast(d); });
        else kloop([](float d) { return sigmoid_from_neg(d); });

        float hl[NT];
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        vnet16_units4849(img, lane_e >> 5, reinterpret_cast<float *>(tbase) + 4 * (lane_e & 15) + (lane_e >> 4), tbase + (lane_e & 31), ch,
                         hl);

#if MVN_FN_PRIO
        __builtin_amdgcn_s_setprio(3);  // tile phase: short, latency-bound bursts
#endif
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int tu = t0 + 16 * u;
            if (tu < T) {  // wave-uniform
                const int nsteps = T - tu < 16 ? T - tu : 16;
                int lane_t = lane;
                asm volatile("" : "+v"(lane_t));
                const int jt = lane_t & 15, qt = lane_t >> 4;
                const int row_addr = 4 * (lane_t & 48);
                const int lane4 = 4 * lane_t;  // ds_bpermute addresses wrap at 64 lanes
                const int4 ul4 = lanes.ldsLane[lane_t];
                const int ulog[4] = {ul4.x, ul4.y, ul4.z, ul4.w};
                const int row_time = row_time_of(qt);
                // the transmitted bits of this row's four symbols (one quad of the image), requested now so the latency hides under layer 3
                const unsigned txq = ldsTx[wave][(tu - s0 + row_time) >> 2];
                float logit[1][4], cost[4];
                vnet16_tile_pass<1>(img, tbase, lane_t, acc + u, hl + u, logit);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    cost[r] = -__int_as_float(__builtin_amdgcn_ds_bpermute(row_addr + 4 * ulog[r], __float_as_int(logit[0][r])));

                float mrec[4];
                mrec[0] = mrec[1] = mrec[2] = mrec[3] = 0.0f;
                if (strict) sweep16_tile<false, true, true>(m, cost, mrec, nsteps, lane4, qt);
                else if (nsteps == 16) sweep16_tile<true, false, true>(m, cost, mrec, nsteps, lane4, qt);
                else sweep16_tile<false, false, true>(m, cost, mrec, nsteps, lane4, qt);
                const float mydec = strict ? decide4<true>(mrec, ulog, jt) : decide4<false>(mrec, ulog, jt);
                const bool mine = jt < 4 && row_time + jt < nsteps;  // lane jt of the row decides symbol tu + row_time + jt
                // (counted in a scalar register: a per-lane count would hold a VGPR across the k-loop)
                nerr += __popcll(__ballot(mine && (int)mydec != (int)((txq >> (jt & 3)) & 1u)));
            }
        }
    }
    // one lane per block reports (the thread index re-read here: nothing lane-derived stays live across the main loop)
    if ((threadIdx.x & 63) == 0)
        mc_add_counters(counters, (unsigned long long)nerr, (unsigned long long)T, nerr ? 1ull : 0ull, 1ull);
}

// Checked arguments only (mvn_vnet_montecarlo_f32).  progress == nullptr: no gate (one round, no stop rule).
inline int launch_vnet_montecarlo(const double *h, int64_t Bh, double sigma, uint64_t seed, int64_t word0, const float *W1, const float *b1,
                                  const float *W2, const float *b2, const float *W3, const float *b3, unsigned long long *counters,
                                  int *progress, int64_t B, int n_rounds, int64_t stop_frame_errors, int T, hipStream_t st) {
    const unsigned grid = (unsigned)((B + kFusedNWaves - 1) / kFusedNWaves);
    for (int r = 0; r < n_rounds; ++r) {
        if (progress) hipLaunchKernelGGL(vnet_mc_gate_kernel, dim3(1), dim3(64), 0, st, counters, progress, (long long)stop_frame_errors);
        hipLaunchKernelGGL(vnet16_mc_kernel, dim3(grid), dim3(64 * kFusedNWaves), 0, st, h, Bh, sigma, (uint32_t)seed, (uint32_t)(seed >> 32),
                           word0 + (int64_t)r * B, W1, b1, W2, b2, W3, b3, counters, (const int *)progress, B, T);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return MVN_OK;
}
