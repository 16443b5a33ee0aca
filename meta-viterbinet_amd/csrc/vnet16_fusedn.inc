// vnet16_fusedn.inc -- fused ViterbiNet detector for 16 states, NT 16-symbol tiles per super-tile (included by
// mvn_hip.hip after vnet16_common.inc, which holds the unit's arithmetic: weight image, k-loop, tile pass, sweep, decisions).
//
// One wavefront owns one block (word) for all T symbols; a workgroup is 8 independent waves sharing one LDS image of the
// weights.  Arithmetic and operation order are those of the reference (exact k-ordered fmaf chains, SLEEF sigmoid), so logits
// and decisions stay bit-identical; what this file decides is how the work is laid on the SIMD (DESIGN.md 5.0-5.1):
//   * NT tiles (16 NT consecutive symbols of the block) are in flight per wave.  NT = 2 needs 24 accumulator VGPRs
//     instead of 48; with the per-lane constants of each phase recomputed or fetched from LDS instead of held, the kernel fits
//     80 VGPRs = 6 waves per SIMD (3 workgroups of 8 waves per CU, 35 KB of LDS each) without scratch.  More waves hide each
//     other's latencies (a lone wave runs at 56 % of the SIMD's rate, four in lock-step at 85 %), and 10 000 blocks are 1.63
//     rounds of 6144 wave slots (profiles/r02_wave_timeline_*.txt).
//   * hidden-2 units 0..47: 3 row tiles x NT symbol tiles of v_mfma_f32_16x16x4_f32 per k-step;
//   * hidden-2 units 48,49: on the vector ALU.  f32 MFMA and every other VALU instruction exclude each other on a gfx950
//     SIMD (profiles/r02_ubench3_mfma_valu_roles.txt) but LDS instructions cost that pipe nothing, so the k-step's
//     sigmoids go through a wave-private LDS image [symbol][k-phase] (NT ds_write_b32), lane L reads back the four k's
//     of ITS symbol (one ds_read_b128) ONE k-step later, and a k-ordered chain of four v_fmac_f32 (the MFMA's fmaf
//     chain, bit for bit) accumulates the unit.  NT = 4: lane = symbol, two chains per lane; NT = 2: lanes 0..31 own
//     unit 48 and lanes 32..63 unit 49 of symbol (lane & 31).
//   * the results go back to the layer-3 operand layout (row q = k-phase) through the same LDS image, and so do the
//     (q,r) transposes of the D-layout tiles.
// Layer 3, the in-place DPP sweep and the decisions are per 16-symbol tile, as in vnet16_common.inc.
#ifndef MVN_FN_WAVES
#define MVN_FN_WAVES 8  // waves (= blocks) per workgroup, sharing one LDS image of the weights
#endif
#ifndef MVN_FN_PRIO
#define MVN_FN_PRIO 1   // wave-priority rules of the main loop (0 = off, for A/B runs)
#endif
#ifndef MVN_FN_WGS
#define MVN_FN_WGS 3    // workgroups per CU the NT = 2 kernel is built for: MVN_FN_WAVES * MVN_FN_WGS / 4 waves per SIMD
#endif
constexpr int kFusedNWaves = MVN_FN_WAVES;

template <int NT>
struct FusedNCfg {
    // second launch bound = waves per SIMD the kernel is built for (hipcc's meaning of the argument): 5 need <= 96 VGPRs
    static constexpr int kMinWgPerCu = NT <= 2 ? (MVN_FN_WAVES * MVN_FN_WGS + 3) / 4 : 4;
};

template <bool WRITE_LOGITS, int NT>
__global__ __launch_bounds__(64 * kFusedNWaves, FusedNCfg<NT>::kMinWgPerCu) void vnet16_fusedn_kernel(
    const float *__restrict__ y, int64_t y_ld, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ logits_out,
    float *__restrict__ final_metric, int64_t B, int T, const float *__restrict__ tx, int64_t tx_ld, int K,
    const unsigned char *__restrict__ row_mask, unsigned long long *__restrict__ counters) {
    static_assert(NT == 2 || NT == 4, "NT = 2 (one unit chain per lane) or 4 (two)");
    constexpr int S = 16;
    constexpr int kSym = 16 * NT;                     // symbols per super-tile
    __shared__ Vnet16Image img;                       // the weights (vnet16_common.inc)
    constexpr int kTImg = kSym > 80 ? kSym : 80;      // float4s per wave: [symbol][k-phase] image / [symbol j][20] transpose image
    __shared__ float4 ldsT[kFusedNWaves][kTImg];      // wave-private scratch image (two uses, see below)
    __shared__ Vnet16LaneStates lanes;                // per lane: logical state of lane (l & 15) at phases 0..3 (kept out of the VGPRs)

#ifdef MVN_DIAG_STAMPS  // diagnostic build only (tools/ablate_fused.py): wave timeline written over the final-metric rows
    const unsigned long long st_re = __builtin_amdgcn_s_memrealtime();
#endif
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: row pointers stay in SGPRs
    const int j = lane & 15;
    const int q = lane >> 4;

    const bool odd_w = img.stage(W1, b1, W2, b2, W3, b3);
    lanes.stage();
    const bool strict = __syncthreads_or(odd_w) != 0;  // the prologue's barrier; workgroup-uniform
    const float wmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[0])));
    const float bmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[1])));

    const int64_t b = (int64_t)blockIdx.x * kFusedNWaves + wave;
    if (b >= B) return;  // whole wave; no barriers below
#ifdef MVN_DIAG_STAMPS
    const unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    float4 *const tbase = &ldsT[wave][0];

    const float *yb = y + b * y_ld;
    float *decb = dec ? dec + b * dec_ld : nullptr;
    const bool counted = tx != nullptr && (row_mask == nullptr || row_mask[b] != 0);
    const float *txb = counted ? tx + b * tx_ld : nullptr;
    int nerr = 0;
    float m = 0.0f;

    float ynext[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int t = 16 * u + sym_time_of(j);
        ynext[u] = yb[t < T ? t : T - 1];
    }
    // Wave priorities (s_setprio).  The SIMD's arbiter serves the oldest wave first: waves that start together finish one
    // after the other, and the last wave of a launch runs alone at 56 % of the rate the SIMD reaches with company
    // (profiles/r02_wave_timeline_*).  Two rules, measured together at -4 % (tools/ablate_fused.py, MVN_FN_PRIO=0 turns them off):
    //  * the tile phase (layer 3, sweep, decisions: short dependent bursts between LDS round trips) runs at the top
    //    priority, so that it is not queued behind other waves' bulk k-loop work and its latency stays off the pipe;
    //  * in the k-loop a wave's priority falls with its progress through the block (thirds: 2, 1, 0), so the waves of a
    //    SIMD finish together instead of in age order.
#ifdef MVN_DIAG_PHASES  // diagnostic build only (tools/diag_phases.py): cycles in the k-loop / in the tile phase, summed
    unsigned long long dgk = 0, dgt = 0, dg_t;
    const unsigned long long dg_t0 = __builtin_amdgcn_s_memtime(), dg_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int third = (T + 2) / 3;
    for (int t0 = 0; t0 < T; t0 += kSym) {
#ifdef MVN_DIAG_PHASES
        dg_t = __builtin_amdgcn_s_memtime();
#endif
#if MVN_FN_PRIO
        if (t0 < third) __builtin_amdgcn_s_setprio(2);
        else if (t0 < 2 * third) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
#endif
        // the k-loop's per-lane LDS addresses are derived here from an opaque copy of the lane id, once per super-tile, so
        // that they do not occupy registers (or scratch) across the tile phase
        int lane_k = lane;
        asm volatile("" : "+v"(lane_k));
        const int qk = lane_k >> 4;
        float *const tbw = reinterpret_cast<float *>(tbase) + 4 * (lane_k & 15) + qk;    // + 64 u: (symbol 16u + j, k-phase q)
        float4 *const tbr = tbase + (NT == 4 ? lane_k : (lane_k & 31));                   // this lane's chain symbol
        const int cunit = NT == 4 ? 0 : (lane_k >> 5);                                    // NT = 2: this lane's unit 48 + cunit
        float yv[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            yv[u] = ynext[u];
            const int tn = t0 + kSym + 16 * u + sym_time_of(lane_k & 15);
            ynext[u] = yb[tn < T ? tn : T - 1];
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
        float ch[NT == 4 ? 2 : 1] = {};  // unit chain(s): NT = 4 -> lane = symbol, units 48 and 49; NT = 2 -> symbol lane & 31, unit 48 + (lane >> 5)
        // (called through a lambda of this kernel, like the sigmoid: see vnet16_kloop)
        auto kloop = [&](auto sig) { vnet16_kloop<NT, true>(sig, img, yv, lane_k, cunit, tbw, tbr, acc, ch); };
        if (fast) kloop([](float d) { return sigmoid_from_neg_fast(d); });
        else kloop([](float d) { return sigmoid_from_neg(d); });

        // units 48,49 -> bias + ReLU -> back through the image: tile u's operand wants h2[48 + q] of symbol (16u + j) at row q
        float hl[NT];
        int lane_e = lane;  // (the epilogue's addresses from a fresh opaque copy of the lane id: the k-loop keeps only what it reads itself)
        asm volatile("" : "+v"(lane_e));
        vnet16_units4849(img, NT == 4 ? 0 : (lane_e >> 5), reinterpret_cast<float *>(tbase) + 4 * (lane_e & 15) + (lane_e >> 4),
                         tbase + (NT == 4 ? lane_e : (lane_e & 31)), ch, hl);

#ifdef MVN_DIAG_PHASES
        {
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();
            dgk += now_ - dg_t;
            dg_t = now_;
        }
#endif
#if MVN_FN_PRIO
        __builtin_amdgcn_s_setprio(3);  // tile phase: short, latency-bound bursts
#endif
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int tu = t0 + 16 * u;
            if (tu < T) {  // wave-uniform
                const int nsteps = T - tu < 16 ? T - tu : 16;
                // Per-lane constants of the tile phase are NOT kept in registers across the k-loop (80 VGPRs = 6 waves per SIMD
                // leave no room): the lane id is made opaque so that the addresses are recomputed here, and the lane's four
                // logical states come back from a 1-KB LDS table (LDS instructions cost the FP32 pipe nothing).
                int lane_t = lane;
                asm volatile("" : "+v"(lane_t));
                const int jt = lane_t & 15, qt = lane_t >> 4;
                const int row_addr = 4 * (lane_t & 48);
                const int lane4 = 4 * lane_t;  // ds_bpermute addresses wrap at 64 lanes
                const int4 ul4 = lanes.ldsLane[lane_t];
                const int ulog[4] = {ul4.x, ul4.y, ul4.z, ul4.w};
                const int row_time = row_time_of(qt);
                const int tdec = tu + row_time + jt;  // the symbol this lane decides (lanes j < 4 of each row)
                float txv = 0.0f;  // its transmitted bit, requested now so the latency hides under layer 3
                if (counted && jt < 4 && tdec < K) txv = txb[tdec];
                float logit[1][4], cost[4];
                vnet16_tile_pass<1>(img, tbase, lane_t, acc + u, hl + u, logit);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (WRITE_LOGITS) {
                        const int tl = tu + row_time + r;
                        if (tl < T) logits_out[((int64_t)b * T + tl) * S + jt] = logit[0][r];
                    }
                    cost[r] = -__int_as_float(__builtin_amdgcn_ds_bpermute(row_addr + 4 * ulog[r], __float_as_int(logit[0][r])));
                }

                float mrec[4];
                mrec[0] = mrec[1] = mrec[2] = mrec[3] = 0.0f;
                // (strict: a non-finite or huge weight, torch.min's NaN rule of vnet16_common.inc)
                if (strict) sweep16_tile<false, true, true>(m, cost, mrec, nsteps, lane4, q);
                else if (nsteps == 16) sweep16_tile<true, false, true>(m, cost, mrec, nsteps, lane4, q);
                else sweep16_tile<false, false, true>(m, cost, mrec, nsteps, lane4, q);
                const float mydec = strict ? decide4<true>(mrec, ulog, jt) : decide4<false>(mrec, ulog, jt);
                const bool mine = jt < 4 && row_time + jt < nsteps;
                if (mine && decb) decb[tdec] = mydec;
                // (counted in a scalar register: a per-lane count would hold a VGPR across the k-loop)
                if (counted) nerr += __popcll(__ballot(mine && tdec < K && (long long)mydec != (long long)txv));
            }
        }
#ifdef MVN_DIAG_PHASES
        dgt += __builtin_amdgcn_s_memtime() - dg_t;
#endif
    }

#ifdef MVN_DIAG_PHASES
    if (final_metric && (threadIdx.x & 63) == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(final_metric + b * S);
        o[0] = dgk;
        o[1] = dgt;
        o[5] = (unsigned long long)((T + kSym - 1) / kSym);
        o[7] = ((__builtin_amdgcn_s_memtime() - dg_t0) << 24) | ((__builtin_amdgcn_s_memrealtime() - dg_r0) & 0xffffff);
    }
    return;
#endif
    if (counted) {  // two global atomics per block in error; the bits/frames totals come from count_totals_kernel
        if ((threadIdx.x & 63) == 0 && nerr) {  // (thread index re-read here: nothing lane-derived stays live across the main loop)
            atomicAdd(&counters[0], (unsigned long long)nerr);
            atomicAdd(&counters[2], 1ull);
        }
    }
#ifdef MVN_DIAG_STAMPS
    if (final_metric && (threadIdx.x & 63) == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(final_metric + b * S);
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        o[0] = __builtin_amdgcn_s_memtime() - st_t0;
        o[1] = __builtin_amdgcn_s_memrealtime() - st_r0;
        o[2] = st_re;
        o[3] = st_r0;
        o[4] = ((unsigned long long)xcc << 32) | hw;
    }
#else
    int lane_f = lane;  // (opaque: nothing the prologue derived from the lane id is kept across the main loop for this)
    asm volatile("" : "+v"(lane_f));
    if (final_metric && lane_f < 16) final_metric[b * S + logical_state(lane_f, T & 3)] = m;  // row 0 holds the metrics
#endif
}
