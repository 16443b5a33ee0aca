// vnet16_coop.inc -- the ViterbiNet detector at 16 states for SMALL batches (included by mvn_hip.hip after vnet16_fusedn.inc).
//
// vnet16_fusedn_kernel gives every block ONE wave: the right shape when thousands of blocks fill the chip, but a lone wave
// runs at 56 % of a SIMD's rate and a block's T symbols are then a T x 344 ns serial chain (0.34 ms for T = 1000, 42 us for
// the by-word evaluation's B = 1, T = 136 call).  The only serial part of the detector is the trellis sweep; the likelihood
// MLP is independent per symbol.  Here a whole 16-wave workgroup serves one block:
//   phase 1  every wave takes 16-symbol tiles round-robin and runs the fused kernel's MLP (vnet16_common.inc: k-ordered fmaf
//            chains, MFMA for hidden units 0..47, the v_fmac chain through LDS for units 48, 49, layer 3 transposed), one tile in flight,
//            and writes the branch costs -logit[t][state] to an LDS buffer (64 B per symbol);
//   phase 2  after one barrier, wave 0 sweeps the T symbols (in-place DPP recurrence, v_permlane*_swap row hand-off -- the
//            code of the fused kernel) reading each step's costs from LDS, and wave 1 follows one tile behind with the
//            DPP decisions (a third of a tile's instructions, off the block's serial chain).
// Same arithmetic in the same order per symbol and per trellis step, so decisions, logits and final metrics are bit-identical
// to the fused kernel's and to the oracle's.  Used for B <= kCoopMaxBlocks and T <= kCoopMaxT (the cost buffer must fit LDS).
constexpr int kCoopWaves = 16;
constexpr int kCoopMaxT = 1024;       // 64 KB of costs next to the 45 KB of weights and per-wave scratch
constexpr int kCoopMaxBlocks = 768;   // three rounds of one workgroup per CU; at ~1000 blocks the one-wave-per-block kernel catches up

// The detector of ONE block by the calling 16-wave workgroup; W1..b3 are this block's weights (the by-word step kernel of
// byword_step.inc gives every block its own set).  After the barrier that ends phase 1 wave 0 runs the trellis recurrence
// and wave 1 turns the metrics it records into decisions: sink(tdec, dec, live) is called by lanes j < 4 of WAVE 1 once per
// 16-symbol tile with the decision of symbol tdec (live = inside the block).  Returns the calling wave's role: kCoopIdle
// (waves 2..15: nothing left to do), kCoopSwept (wave 0: *m_out = the block's final path metric, in its row-0 lanes),
// kCoopDecided (wave 1: every sink call has been made).
// SURV (the by-word step's traced-back decision, byword_step.inc): the running-argmin decisions are not taken and sink is never
// called.  Wave 0 hands over a = recorded metric + branch cost of its four steps instead of the recorded metrics (four adds per tile
// off the chain, the same sums the steps formed), wave 1 turns them into the tile's survivor words surv_words[16 tile ..]
// (surv16_tile_store) and, once wave 0 has left the final metric in fm[16] (logical state order), returns kCoopDecided: the words of
// steps 0 .. T - 1 and fm are then visible to it.
// KEEP (with SURV; the list step, byword_step.inc): the branch costs stay where phase 1 put them, costs[t][state], and the metrics
// before every step stay as well: wave 0 hands the recorded metrics over through alpha (its lane layout, 1 KB per tile, the same
// floats after costs in the dynamic LDS), wave 1 forms a = metric + cost itself (the same add) and rewrites the tile as
// alpha[t][state].  The caller's dynamic LDS is then 2 KB per tile.
enum { kCoopIdle = 0, kCoopSwept = 1, kCoopDecided = 2 };
template <bool WRITE_LOGITS, bool SURV = false, bool KEEP = false, class Sink>
__device__ __forceinline__ int coop_detect_block(const float *__restrict__ yb, const float *__restrict__ W1,
                                                 const float *__restrict__ b1, const float *__restrict__ W2,
                                                 const float *__restrict__ b2, const float *__restrict__ W3,
                                                 const float *__restrict__ b3, float *__restrict__ logits_b, int T,
                                                 float *m_out, Sink sink, unsigned short *surv_words = nullptr,
                                                 float *fm = nullptr, float **alpha_out = nullptr) {
    static_assert(!KEEP || SURV, "the metrics are kept next to the survivors");
    constexpr int S = 16;
    __shared__ int s_swept;  // tiles whose recorded metrics wave 0 has handed over
    __shared__ Vnet16Image img;              // the weights (vnet16_common.inc)
    __shared__ float4 ldsT[kCoopWaves][80];  // per wave: [symbol][k-phase] image (16 float4) / [symbol j][20] transpose image
    extern __shared__ float costs[];         // [16 * tiles][16]: -logit of (time, state)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15;
    const int q = lane >> 4;

    const bool odd_w = img.stage(W1, b1, W2, b2, W3, b3);
    const bool strict = __syncthreads_or(odd_w) != 0;  // the prologue's barrier; workgroup-uniform
    const float wmax = img.ldsMax[0], bmax = img.ldsMax[1];

    const int tiles = (T + 15) >> 4;
    float *const alpha = costs + tiles * 16 * S;  // (KEEP only)
    if (KEEP) *alpha_out = alpha;
    float4 *const tbase = &ldsT[wave][0];
    const int sym_time = sym_time_of(j), row_time = row_time_of(q);
    const int cunit = (lane >> 4) & 1;  // this lane's unit chain: symbol (lane & 15), unit 48 + cunit (lanes >= 32 duplicate)
    float *const tbw = reinterpret_cast<float *>(tbase) + 4 * j + q;
    float4 *const tbr = tbase + j;

    // ---------------------------------------------------------------- phase 1: the MLP, one 16-symbol tile per wave and trip
    for (int tile = wave; tile < tiles; tile += kCoopWaves) {
        const int tu = 16 * tile;
        const int ty = tu + sym_time;
        const float yv[1] = {yb[ty < T ? ty : T - 1]};
        const bool fast = __all(fabsf(yv[0]) * wmax + bmax <= kFastSigmoidBound);
        f32x4 acc[1][3];
#pragma unroll
        for (int tau = 0; tau < 3; ++tau) acc[0][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ch[1] = {0.0f}, hl[1], logit[1][4];
        if (fast) vnet16_kloop<1, false>([](float d) { return sigmoid_from_neg_fast(d); }, img, yv, lane, cunit, tbw, tbr, acc, ch);
        else vnet16_kloop<1, false>([](float d) { return sigmoid_from_neg(d); }, img, yv, lane, cunit, tbw, tbr, acc, ch);
        vnet16_units4849(img, cunit, tbw, tbr, ch, hl);
        vnet16_tile_pass<1>(img, tbase, lane, acc, hl, logit);
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // lane (state j, row q): time 4 q' + r of the tile
            const int tl = tu + row_time + r;
            if (WRITE_LOGITS && tl < T) logits_b[(int64_t)tl * S + j] = logit[0][r];
            costs[tl * S + j] = -logit[0][r];  // vnet_detector.py:57
        }
    }
    if (threadIdx.x == 0) s_swept = 0;
    __syncthreads();
    if (wave > 1) return kCoopIdle;

    // ---------------------------------------------------------------- phase 2: wave 0 sweeps the block, wave 1 decides
    // The recurrence is the block's serial chain (T dependent add + min steps); the decisions of a tile (four all-reduces
    // of values and of tying indices) depend on the metrics recorded during that tile only, so wave 0 hands them to wave 1
    // through the tile's own 1-KB slot of the cost buffer (its costs are in wave 0's registers by then) and moves on.
    int ulog[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ulog[r] = logical_state(j, r);
    if (wave == 0) {
        float m = 0.0f;
        for (int tile = 0; tile < tiles; ++tile) {
            const int tu = 16 * tile;
            const int nsteps = T - tu < 16 ? T - tu : 16;
            float cost[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) cost[r] = costs[(tu + row_time + r) * S + ulog[r]];  // the lane's logical state at phase r
            float mrec[4];
            mrec[0] = mrec[1] = mrec[2] = mrec[3] = 0.0f;
            if (strict) sweep16_tile<false, true, false>(m, cost, mrec, nsteps, 0, q);  // torch.min's NaN rule (vnet16_common.inc)
            else if (nsteps == 16) sweep16_tile<true, false, false>(m, cost, mrec, nsteps, 0, q);
            else sweep16_tile<false, false, false>(m, cost, mrec, nsteps, 0, q);
            if (SURV && !KEEP) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mrec[r] += cost[r];
            }
            reinterpret_cast<float4 *>((KEEP ? alpha : costs) + tu * S)[lane] = make_float4(mrec[0], mrec[1], mrec[2], mrec[3]);
            __hip_atomic_store(&s_swept, tile + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        *m_out = m;
        if (SURV) {
            if (q == 0) fm[logical_state(j, T & 3)] = m;
            __hip_atomic_store(&s_swept, tiles + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return kCoopSwept;
    }
    for (int tile = 0; tile < tiles; ++tile) {
        const int tu = 16 * tile;
        const int nsteps = T - tu < 16 ? T - tu : 16;
        const int tdec = tu + row_time + j;
        while (__hip_atomic_load(&s_swept, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= tile) __builtin_amdgcn_s_sleep(1);
        const float4 mr4 = reinterpret_cast<const float4 *>((KEEP ? alpha : costs) + tu * S)[lane];
        const float mrec[4] = {mr4.x, mr4.y, mr4.z, mr4.w};
        if (KEEP) {
            float a[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = mrec[r] + costs[(tu + row_time + r) * S + ulog[r]];
            surv16_tile_store(a, ulog, lane, surv_words + tu);
#pragma unroll
            for (int r = 0; r < 4; ++r) alpha[(tu + row_time + r) * S + ulog[r]] = mrec[r];  // (every lane's read came first)
            continue;
        }
        if (SURV) {
            surv16_tile_store(mrec, ulog, lane, surv_words + tu);
            continue;
        }
        const float mydec = strict ? decide4<true>(mrec, ulog, j) : decide4<false>(mrec, ulog, j);
        if (j < 4) sink(tdec, mydec, row_time + j < nsteps);
    }
    if (SURV) {
        while (__hip_atomic_load(&s_swept, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= tiles) __builtin_amdgcn_s_sleep(1);
        wave_lds_fence();  // (the words are this wave's own LDS writes)
    }
    return kCoopDecided;
}

template <bool WRITE_LOGITS>
__global__ __launch_bounds__(64 * kCoopWaves, 4) void vnet16_coop_kernel(
    const float *__restrict__ y, int64_t y_ld, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ logits_out,
    float *__restrict__ final_metric, int64_t B, int T, const float *__restrict__ tx, int64_t tx_ld, int K,
    const unsigned char *__restrict__ row_mask, unsigned long long *__restrict__ counters) {
    const int64_t b = blockIdx.x;  // one block per workgroup
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    float *decb = dec ? dec + b * dec_ld : nullptr;
    const bool counted = tx != nullptr && (row_mask == nullptr || row_mask[b] != 0);
    const float *txb = counted ? tx + b * tx_ld : nullptr;
    int nerr = 0;
    float m = 0.0f;
    const int role = coop_detect_block<WRITE_LOGITS>(
        y + b * y_ld, W1, b1, W2, b2, W3, b3, WRITE_LOGITS ? logits_out + b * (int64_t)T * 16 : nullptr, T, &m,
        [&](int tdec, float mydec, bool live) {
            if (!live) return;
            if (decb) decb[tdec] = mydec;
            if (counted && tdec < K) nerr += ((long long)mydec != (long long)txb[tdec]) ? 1 : 0;
        });
    if (role == kCoopDecided && counted) {  // wave 1 holds the decisions' error count
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nerr += __shfl_xor(nerr, off);
        if (lane == 0 && nerr) {
            atomicAdd(&counters[0], (unsigned long long)nerr);
            atomicAdd(&counters[2], 1ull);
        }
    }
    if (role == kCoopSwept && final_metric && q == 0) final_metric[b * 16 + logical_state(j, T & 3)] = m;
}
