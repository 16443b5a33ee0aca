// vnet16_dealt.inc -- the fused 16-state ViterbiNet detector with its work dealt in 32-symbol UNITS instead of whole blocks
// (included by mvn_hip.hip after vnet16_fusedn.inc; the unit's arithmetic -- k-loop, tile pass, sweep, decisions -- is vnet16_common.inc's).
//
// vnet16_fusedn_kernel gives every block to one wave.  A block of 1000 symbols is 0.8 ms of a wave's life at 6 waves per SIMD, so
// the launch is quantised in blocks: BASELINE's 10 000 blocks are 9.77 per SIMD -- ten on most, in a 6-wave round and a 4-wave
// round that runs the SIMD below its rate -- and a launch of 1 250 or 2 048 blocks leaves most wave slots empty (DESIGN.md 5.1:
// 327 cycles per symbol and SIMD at 10 000 blocks against 311 in steady state; 423 at 2 048 blocks).  Only the trellis sweep is
// sequential within a block; its state is 16 path metrics.  Here the chip's 3 x CUs workgroups ("groups" of 8 waves) share ALL the
// launch's units evenly:
//   * the launch's units -- block-major, U = ceil(T / 32) per block -- are cut into n_groups equal contiguous ranges (McNaughton's
//     wrap-around rule: no range is shorter than a block, so a block lies in at most two of them);
//   * a group executes its range in the order [head of the block that continues in the NEXT group] [whole blocks] [tail of the
//     block that began in the PREVIOUS group], and deals the units of that order round-robin to its 8 waves;
//   * a wave runs a unit's MLP (the k-loop: 95 % of the work, independent of every other unit), THEN takes the block's path metrics
//     from the wave that swept the unit before it -- through LDS within the group (a sequence number per slot, an acknowledgement
//     before a slot is reused), through one 128-byte line of the caller's workspace between groups -- sweeps its 32 steps and passes
//     the metrics on.  The cross-group wait is for a unit the OTHER group executes first and this group last: it has been over for
//     most of the launch when it is looked at.  It points to the lower-numbered group, which the dispatcher started no later; the
//     spin is bounded all the same (status word + NaN decisions if abandoned: never seen).
// Every SIMD then carries the same number of units, all its wave slots stay busy to the end, and a launch of B >= n_groups blocks
// keeps n_groups x 8 waves busy whatever B is.  Arithmetic per symbol and per trellis step is the fused kernel's: bit-identical.
#ifndef MVN_DEALT_PMODE
#define MVN_DEALT_PMODE 0
#endif
#ifndef MVN_DEALT_P1N  // the k-loop's priority falls from 2 to 1 at P1N / P1D of a wave's units and to 0 at P2N / P2D
#define MVN_DEALT_P1N 1  // (1/2 and 3/4 measured best: thirds -0.7 %, later or earlier thresholds and per-unit cyclic priorities worse;
#define MVN_DEALT_P1D 2  //  profiles/r05_dealt_prio*.txt)
#define MVN_DEALT_P2N 3
#define MVN_DEALT_P2D 4
#endif
constexpr int kDealtWaves = 8;
constexpr int kDealtUnit = 32;              // symbols per unit (two 16-symbol tiles)
constexpr int kDealtLineFloats = 32;        // one 128-byte line per group in the workspace: dwords 0..15 the metrics, 16 abandoned, 17 the
                                            // carry of bit errors, 18-19 / 20-21 the 64-bit flags of the metrics / of the carry.  A flag is
                                            // SET when it holds the launch's nonce (a fresh 64-bit number per launch, mvn_hip.hip):
                                            // nothing has to be cleared between launches, whatever the workspace held before
                                            // (a graph-captured launch replays with ONE nonce: its launcher clears the lines, mvn_hip.hip)
constexpr unsigned kDealtSpinLimit = 1u << 21;  // x ~2 us per poll

// bytes of workspace a dealt launch of n_rings rings needs: line 0 = {status}, line 1 + r = ring r's hand-off to ring r + 1
inline size_t dealt_workspace_bytes(int n_rings) { return (size_t)(n_rings + 1) * kDealtLineFloats * sizeof(float); }

// SURV (round 5): the sweep's survivors as well (mvn_vnet_decode_surv_f32: ViterbiNet with survivor-path traceback without the logits
// in HBM).  They are worked out in pass C, OFF the hand-off chain: a row has recorded the metrics before its four steps and still
// holds their costs, so every row re-forms its four stages' candidates at once -- a = m + cost, the partner's through the stage's DPP
// operation -- and the lanes that hold an even predecessor apply torch.min's index rule (first NaN, else strictly smaller); the
// step's 16-bit word (bits s' and s' + 8 of the new state) is OR-ed over the row's 16 lanes by four DPP steps and lane 0 of the row
// stores the row's four words, 8 bytes.  (36 vector instructions per 16 steps.)
template <bool WRITE_LOGITS, bool SURV = false>
__global__ __launch_bounds__(64 * kDealtWaves, SURV ? 5 : 6) void vnet16_dealt_kernel(
    const float *__restrict__ y, int64_t y_ld, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ logits_out,
    float *__restrict__ final_metric, int B, int T, const float *__restrict__ tx, int64_t tx_ld, int K,
    const unsigned char *__restrict__ row_mask, unsigned long long *__restrict__ counters, float *__restrict__ ws, int n_groups,
    int ring, unsigned spin_limit, int skip_publish_ring, unsigned long long nonce, unsigned char *__restrict__ surv) {
    constexpr int NT = 2;
    constexpr int S = 16;
    constexpr int kSym = 16 * NT;
    __shared__ Vnet16Image img;                 // the weights (vnet16_common.inc)
    __shared__ float4 ldsT[kDealtWaves][160];   // per wave: the [symbol][k-phase] image of the k-loop / two [symbol j][20] transposition images
    __shared__ Vnet16LaneStates lanes;
    __shared__ float ldsHand[kDealtWaves][20];  // slot w: the path metrics (row-0 lane order) wave w last published, [16] = abandoned
    __shared__ int ldsSeq[kDealtWaves];         // ... for the unit with this execution number + 1
    __shared__ int ldsCarry[kDealtWaves];       // counting launches: the block's bit errors up to and including that unit ...
    __shared__ int ldsSeqC[kDealtWaves];        // ... published at the unit's END (the metrics leave right after its sweep)
    __shared__ int ldsAck[kDealtWaves];         // the number the slot's consumer has taken (everything it wanted of it)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 15;

    const bool odd_w = img.stage(W1, b1, W2, b2, W3, b3);
    lanes.stage();
    if (threadIdx.x < kDealtWaves) {
        ldsSeq[threadIdx.x] = 0;
        ldsSeqC[threadIdx.x] = 0;
        ldsAck[threadIdx.x] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<int *>(ws) = 0;  // the status word (an abandoned wait sets it, seconds later)
    const bool strict = __syncthreads_or(odd_w) != 0;  // the prologue's barrier; workgroup-uniform.  No barrier below.
    const float wmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[0])));
    const float bmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[1])));

    // ---- this ring's range of the launch's units and the order it executes them in (all wave-uniform: scalar registers).
    // A ring is `ring` = 8, 4, 2 or 1 consecutive waves of the workgroup: ring 4 = one wave per SIMD, all of the same age on it.
    const int rings_per_group = kDealtWaves / ring;
    const int rpos = wave % ring, rbase = wave - rpos;              // this wave's place in its ring; the ring's first wave
    const int ring_g = (int)blockIdx.x * rings_per_group + wave / ring;
    const int n_rings = n_groups * rings_per_group;
    const int U = (T + kDealtUnit - 1) / kDealtUnit;
    const long long N = (long long)B * U;
    const int lo = (int)(N * ring_g / n_rings), hi = (int)(N * (ring_g + 1) / n_rings);
    const int n = hi - lo;
    const int n_head = hi % U;                         // units of the block that continues in the next ring: executed FIRST
    const int n_tail = (lo % U) ? U - lo % U : 0;      // units of the block that began in the previous ring: executed LAST
    const int n_mid = n - n_head - n_tail;             // whole blocks in between
    auto unit_pos = [&](int e) { return e < n_head ? hi - n_head + e : e < n_head + n_mid ? lo + n_tail + (e - n_head) : lo + (e - n_head - n_mid); };

    float4 *const tbase = &ldsT[wave][0];
    const int q = lane >> 4;

#ifdef MVN_DIAG_PHASES  // diagnostic build only (tools/diag_phases.py): cycles per phase, summed over the wave's units
    unsigned long long dg[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long dg_t;
    const unsigned long long dg_t0 = __builtin_amdgcn_s_memtime(), dg_r0 = __builtin_amdgcn_s_memrealtime();
#define MVN_DG_START() dg_t = __builtin_amdgcn_s_memtime()
#define MVN_DG_LAP(I)                                                 \
    {                                                                 \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        dg[I] += now_ - dg_t;                                         \
        dg_t = now_;                                                  \
    }
#else
#define MVN_DG_START()
#define MVN_DG_LAP(I)
#endif
    int last_pub = 0;  // sequence number of this wave's last in-group publication (0: none yet)
    float ynext[NT];
    // the wave's current unit: position in the launch's block-major order, block, unit within the block.  A wave's units are 8
    // apart in its group's execution order, so within a segment the next position is this one + 8: the division by U is only
    // taken where the order jumps (head -> whole blocks -> tail)
    int pos = rpos < n ? unit_pos(rpos) : 0;
    int b = pos / U, s = pos - b * U;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int t = s * kDealtUnit + 16 * u + sym_time_of(j);
        ynext[u] = rpos < n ? y[(int64_t)b * y_ld + (t < T ? t : T - 1)] : 0.0f;
    }
    // what travels along a block: the path metrics, "a hand-off before this was abandoned", the bit errors so far (counting
    // launches).  A ring of ONE wave keeps them in registers from unit to unit.
    float m = 0.0f;
    bool bad = false;
    int carry = 0;

    for (int e = rpos; e < n; e += ring) {
        const int t0 = s * kDealtUnit;
        int pos2 = pos, b2 = b, s2 = s;  // this wave's next unit
        if (e + ring < n) {
            pos2 = unit_pos(e + ring);
            if (pos2 == pos + ring) {
                s2 = s + ring;
                while (s2 >= U) {
                    s2 -= U;
                    ++b2;
                }
            } else {
                b2 = pos2 / U;
                s2 = pos2 - b2 * U;
            }
        }
        const float *yb = y + (int64_t)b * y_ld;
        float *decb = dec ? dec + (int64_t)b * dec_ld : nullptr;
        const bool counted = tx != nullptr && (row_mask == nullptr || row_mask[b] != 0);
        const float *txb = counted ? tx + (int64_t)b * tx_ld : nullptr;
        int nerr = 0;
        const bool own_prev = ring == 1 && s > 0 && e != n_head + n_mid;  // the block's previous unit was this wave's previous unit
        if (!own_prev) m = 0.0f, bad = false, carry = 0;
#ifdef MVN_DIAG_PHASES
        if (e != rpos) MVN_DG_LAP(5)  // from the end of the previous unit to here
#endif
        MVN_DG_START();
        const bool counting = tx != nullptr;  // (launch-uniform) the carry of bit errors travels along the block too

#if MVN_FN_PRIO
        // As in the one-wave-per-block kernel, a wave's k-loop priority falls with its progress (thirds of its units: 2, 1, 0).  The
        // arbiter serves the oldest wave first: without the rule the group dispatched first to a SIMD runs ahead and the last one
        // finishes alone, at a fraction of the SIMD's rate (measured at 6 144 blocks: mean wave lifetime 707 us, longest 896 us).
#if MVN_DEALT_PMODE == 0
        if (MVN_DEALT_P1D * e < MVN_DEALT_P1N * n) __builtin_amdgcn_s_setprio(2);
        else if (MVN_DEALT_P2D * e < MVN_DEALT_P2N * n) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
#elif MVN_DEALT_PMODE == 1  // by the units the wave has left
        {
            const int left = (n - e + ring - 1) / ring;
            if (left > MVN_DEALT_P1N) __builtin_amdgcn_s_setprio(2);
            else if (left > MVN_DEALT_P2N) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
#else  // cyclic
        {
            const int c = (e / ring) % 3;
            if (c == 0) __builtin_amdgcn_s_setprio(2);
            else if (c == 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
#endif
#endif
        int lane_k = lane;
        asm volatile("" : "+v"(lane_k));
        const int qk = lane_k >> 4;
        float *const tbw = reinterpret_cast<float *>(tbase) + 4 * (lane_k & 15) + qk;
        float4 *const tbr = tbase + (lane_k & 31);
        const int cunit = lane_k >> 5;  // this lane's unit chain: symbol (lane & 31), unit 48 + cunit
        float yv[NT];
        {
            const float *yb2 = y + (int64_t)b2 * y_ld;  // the next unit's samples are requested now
            const int t02 = s2 * kDealtUnit;
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                yv[u] = ynext[u];
                const int tn = t02 + 16 * u + sym_time_of(lane_k & 15);
                ynext[u] = yb2[tn < T ? tn : T - 1];
            }
        }
        float ymax = fmaxf(fabsf(yv[0]), fabsf(yv[1]));
        const bool fast = __all(ymax * wmax + bmax <= kFastSigmoidBound);

        f32x4 acc[NT][3];
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int tau = 0; tau < 3; ++tau) acc[u][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ch[1] = {0.0f};
        // the unit's live tiles: a block's last unit may end within its first tile (T = 1000: 8 symbols), and then runs the
        // k-loop for that tile alone -- half the MFMAs and sigmoids (tile 1's accumulators stay 0; nothing of tile 1 is used)
        const bool one_tile = t0 + 16 >= T;
        if (fast && !one_tile) vnet16_kloop<2, true>([](float d) { return sigmoid_from_neg_fast(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
        else if (!one_tile) vnet16_kloop<2, true>([](float d) { return sigmoid_from_neg(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
        else if (fast) vnet16_kloop<1, true>([](float d) { return sigmoid_from_neg_fast(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
        else vnet16_kloop<1, true>([](float d) { return sigmoid_from_neg(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);

        float hl[NT];
        vnet16_units4849(img, cunit, tbw, tbr, ch, hl);

#if MVN_FN_PRIO
        __builtin_amdgcn_s_setprio(3);
#endif
        MVN_DG_LAP(0)
        // The tile phase in three passes, so that the block's chain of hand-offs holds nothing but the two sweeps:
        //   A  per tile: bias + ReLU, the (q, r) transposes, layer 3, the logits' way into the sweep's lane order -- needs no metrics;
        //   B  take the metrics, sweep tile 0 and tile 1 (32 dependent add + min_dpp steps, 8 row hand-offs), pass them on;
        //   C  per tile: the decisions from the recorded metrics, their stores, the error count -- nobody waits for these.
        // (With the whole tile phase inside the chain a group's eight units could only follow each other every ~8.7 k cycles:
        // the chain, not the pipes, set the pace -- 362 cycles per symbol and SIMD against the one-wave-per-block kernel's 312.)
        const int n0 = T - t0 < 16 ? T - t0 : 16;                                   // live steps of tile 0 (>= 1)
        const int n1 = T - t0 - 16 < 0 ? 0 : (T - t0 - 16 < 16 ? T - t0 - 16 : 16);  // ... of tile 1 (0: the block ends in tile 0)
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int jt = lane_t & 15, qt = lane_t >> 4;
        const int lane4 = 4 * lane_t;
        const int4 ul4 = lanes.ldsLane[lane_t];
        const int ulog[4] = {ul4.x, ul4.y, ul4.z, ul4.w};
        const int row_time = row_time_of(qt);
        float cost[NT][4], mrec[NT][4], txv[NT];
        // ---- pass A, both tiles together (two transposition images per wave, the two layer-3 chains interleaved: the phase is
        // latency, not work).  Tile 1 is evaluated even when the block ended in tile 0 (n1 == 0): nothing of it is stored or swept.
        {
            const int row_addr = 4 * (lane_t & 48);
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int tdec = t0 + 16 * u + row_time + jt;
                txv[u] = 0.0f;
                if (counted && jt < 4 && tdec < K) txv[u] = txb[tdec];
#pragma unroll
                for (int r = 0; r < 4; ++r) mrec[u][r] = 0.0f;
            }
            float logit[NT][4];
            vnet16_tile_pass<NT>(img, tbase, lane_t, acc, hl, logit);
#pragma unroll
            for (int u = 0; u < NT; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (WRITE_LOGITS) {
                        const int tl = t0 + 16 * u + row_time + r;
                        if (tl < T) logits_out[((int64_t)b * T + tl) * S + jt] = logit[u][r];
                    }
                    cost[u][r] = -__int_as_float(__builtin_amdgcn_ds_bpermute(row_addr + 4 * ulog[r], __float_as_int(logit[u][r])));
                }
        }

        MVN_DG_LAP(1)
        // ---- pass B: the block's path metrics from the wave that swept its previous unit ...
        if (s > 0 && !own_prev) {
            if (e != n_head + n_mid) {  // within the ring, through LDS
                const int pw = rbase + (rpos + ring - 1) % ring;
#ifndef MVN_DEALT_NOWAIT  // (diagnostic builds only: wrong results, the cost of the coupling by difference)
                while (__hip_atomic_load(&ldsSeq[pw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != e) __builtin_amdgcn_s_sleep(1);
#endif
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                m = ldsHand[pw][jt];
                bad = __builtin_amdgcn_readfirstlane(__float_as_int(ldsHand[pw][16])) != 0;
                if (!counting) {  // (a counting launch acknowledges after it has read the carry as well)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the reads above have returned
                    if (lane_t == 0) __hip_atomic_store(&ldsAck[pw], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {  // (s > 0 at the first unit after the whole blocks: the tail of the block the previous group began)
                const float *line = ws + (size_t)ring_g * kDealtLineFloats;  // line 1 + (ring_g - 1)
                const unsigned long long *flag = reinterpret_cast<const unsigned long long *>(line) + 9;
                unsigned spins = 0;
                bool ok = true;
                while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nonce) {
                    __builtin_amdgcn_s_sleep(32);
                    if (++spins > spin_limit) {
                        ok = false;
                        break;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                m = line[jt];
                bad = !ok || __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(line)[16]) != 0;
                if (!ok && lane_t == 0) __hip_atomic_store(reinterpret_cast<int *>(ws), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        MVN_DG_LAP(2)
        // ... the two sweeps ...
        if (!strict && n1 == 16) {  // (the common case: both tiles whole)
            sweep16_tile<true, false, true>(m, cost[0], mrec[0], 16, lane4, q);
            sweep16_tile<true, false, true>(m, cost[1], mrec[1], 16, lane4, q);
        } else if (!strict) {
            sweep16_tile<false, false, true>(m, cost[0], mrec[0], n0, lane4, q);
            if (n1 > 0) sweep16_tile<false, false, true>(m, cost[1], mrec[1], n1, lane4, q);
        } else {
            sweep16_tile<false, true, true>(m, cost[0], mrec[0], n0, lane4, q);
            if (n1 > 0) sweep16_tile<false, true, true>(m, cost[1], mrec[1], n1, lane4, q);
        }
        // ... and on to the wave that sweeps the block's next unit
        if (s + 1 < U) {
            if (e == n_head - 1) {  // the block continues in the next ring: one line of the workspace
                float *line = ws + (size_t)(1 + ring_g) * kDealtLineFloats;
                if (ring_g != skip_publish_ring) {
                    if (lane_t < 16) line[lane_t] = m;
                    if (lane_t == 16) reinterpret_cast<int *>(line)[16] = bad ? 1 : 0;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the line is visible device-wide before the flag
                    unsigned long long nv = nonce;  // (opaque: the VGPR copy of the nonce is made here, not kept -- or spilled -- across the unit loop)
                    asm volatile("" : "+s"(nv));
                    if (lane_t == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(line) + 9, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else if (ring > 1) {
                if (last_pub) {  // the slot's previous contents have been taken
#ifndef MVN_DEALT_NOWAIT
                    while (__hip_atomic_load(&ldsAck[wave], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != last_pub) __builtin_amdgcn_s_sleep(1);
#endif
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                }
                if (lane_t < 16) ldsHand[wave][lane_t] = m;
                if (lane_t == 16) ldsHand[wave][16] = __int_as_float(bad ? 1 : 0);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                last_pub = e + 1;
                if (lane_t == 0) __hip_atomic_store(&ldsSeq[wave], last_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }

        MVN_DG_LAP(3)
        // ---- pass C: decisions
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            {  // (both tiles unconditionally: one basic block, the two tiles' DPP chains interleave; n1 == 0 stores nothing)
                const int nsteps = u == 0 ? n0 : n1;
                const int tdec = t0 + 16 * u + row_time + jt;
                float mydec = strict ? decide4<true>(mrec[u], ulog, jt) : decide4<false>(mrec[u], ulog, jt);
                if (bad) mydec = __int_as_float(0x7fc00000);  // an abandoned hand-off: no decision is claimed
                if (jt < 4 && row_time + jt < nsteps) {
                    if (decb) decb[tdec] = mydec;
                    if (counted && tdec < K) nerr += ((long long)mydec != (long long)txv[u]) ? 1 : 0;
                }
                if constexpr (SURV) {
                    unsigned wv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float a = mrec[u][r] + cost[u][r];  // the stage's candidate of this lane (acs_inplace<r>)
                        const float pa = r == 0 ? dpp_f32<MVN_DPP_XOR1>(a) : r == 1 ? dpp_f32<MVN_DPP_XOR2>(a)
                                       : r == 2 ? dpp_f32<MVN_DPP_XOR7>(a) : dpp_f32<MVN_DPP_XOR8>(a);
                        // lanes whose logical state at phase r is even hold the predecessor 2 s' of new states s', s' + 8; index 1 iff the
                        // odd candidate is strictly smaller or NaN while the even one is not NaN (torch.min, trellis_utils.py:30)
                        const bool j1 = (ulog[r] & 1) == 0 && a == a && !(pa >= a);
                        int w = j1 ? (int)(0x0101u << (ulog[(r + 1) & 3] & 7)) : 0;
                        w |= dpp_i32<MVN_DPP_XOR1>(w);
                        w |= dpp_i32<MVN_DPP_XOR2>(w);
                        w |= dpp_i32<MVN_DPP_XOR7>(w);
                        w |= dpp_i32<MVN_DPP_XOR8>(w);
                        wv[r] = (unsigned)w;
                    }
                    if (jt == 0 && row_time < nsteps) {  // lane 0 of the row: its four steps' words, 8 bytes when they all exist
                        unsigned char *sp = surv + ((size_t)b * T + t0 + 16 * u + row_time) * 2;
                        if (row_time + 3 < nsteps) {
                            *reinterpret_cast<uint2 *>(sp) = make_uint2(wv[0] | (wv[1] << 16), wv[2] | (wv[3] << 16));
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (row_time + r < nsteps) reinterpret_cast<unsigned short *>(sp)[r] = (unsigned short)wv[r];
                        }
                    }
                }
            }
        }

        MVN_DG_LAP(4)
        // ---- counting launches: the unit's bit errors join the block's carry, which follows the metrics at the unit's end
        if (counting) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nerr += __shfl_xor(nerr, off);
            int total = __builtin_amdgcn_readfirstlane(nerr);
            if (own_prev) {
                total += carry;
            } else if (s > 0) {
                if (e != n_head + n_mid) {
                    const int pw = rbase + (rpos + ring - 1) % ring;
                    while (__hip_atomic_load(&ldsSeqC[pw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != e) __builtin_amdgcn_s_sleep(2);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    total += __builtin_amdgcn_readfirstlane(ldsCarry[pw]);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) __hip_atomic_store(&ldsAck[pw], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (!bad) {  // (after an abandoned wait nothing of that line is waited for again)
                    const int *line = reinterpret_cast<const int *>(ws + (size_t)ring_g * kDealtLineFloats);
                    unsigned spins = 0;
                    while (__hip_atomic_load(reinterpret_cast<const unsigned long long *>(line) + 10, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nonce &&
                           ++spins <= spin_limit)
                        __builtin_amdgcn_s_sleep(32);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    total += __builtin_amdgcn_readfirstlane(line[17]);
                }
            }
            if (s + 1 < U) {
                if (e == n_head - 1) {
                    int *line = reinterpret_cast<int *>(ws + (size_t)(1 + ring_g) * kDealtLineFloats);
                    if (ring_g != skip_publish_ring) {
                        if (lane == 0) line[17] = total;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                        unsigned long long nv = nonce;
                        asm volatile("" : "+s"(nv));
                        if (lane == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(line) + 10, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else if (ring == 1) {
                    carry = total;
                } else {
                    if (lane == 0) ldsCarry[wave] = total;  // (the slot is free: the metrics of this unit went into it above)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) __hip_atomic_store(&ldsSeqC[wave], e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else if (counted && total != 0 && lane == 0) {  // the block ends here: two global atomics per block in error
                atomicAdd(&counters[0], (unsigned long long)total);
                atomicAdd(&counters[2], 1ull);
            }
        }
        if (s + 1 == U && final_metric) {  // (the lane id is made opaque: nothing lane-derived is hoisted out of the unit loop)
            int lane_f = lane;
            asm volatile("" : "+v"(lane_f));
            if (lane_f < 16) final_metric[(int64_t)b * S + logical_state(lane_f, T & 3)] = m;
        }
        pos = pos2, b = b2, s = s2;
    }
#ifdef MVN_DIAG_PHASES
    if (final_metric && (threadIdx.x & 63) == 0 && ((int)blockIdx.x * kDealtWaves + wave) < B) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(final_metric + (int64_t)((int)blockIdx.x * kDealtWaves + wave) * S);
        for (int i = 0; i < 5; ++i) o[i] = dg[i];
        o[5] = (unsigned long long)((n - rpos + ring - 1) / ring);  // units of this wave
        o[6] = dg[5];
        o[7] = ((__builtin_amdgcn_s_memtime() - dg_t0) << 24) | ((__builtin_amdgcn_s_memrealtime() - dg_r0) & 0xffffff);
    }
#endif
}

// ---- The ring-of-one form.  From 8 x groups blocks on every wave is a ring of its own (dealt_plan): it sweeps its own blocks and
// the path metrics never leave its registers except at the two ends of its range.  What vnet16_dealt_kernel pays per unit for
// serving rings of 8, 4, 2 and 1 from one loop body -- the next unit's (pos, b, s) with a division where the order jumps, the row
// pointers, own_prev / one_tile / n0 / n1 / counted, the priority rule's multiplies, the in-group hand-off's code, the partial-tile
// guards of the sweep and of the stores -- is paid here per BLOCK or not at all.  The range executes as runs of one block's units
// in the general form's order: [the head: units 0 .. n_head - 1 of the block that continues in the next ring] [whole blocks] [the
// tail: the last n_tail units of the block the previous ring began].  ONE loop over those runs holds ONE copy of the unit's code --
// a copy per segment would be three times 6 k-loops, 160 KB of code for the 64 KB instruction cache -- and a run is told from its ends:
// s1 < U is the head (it publishes its metrics after its last unit), s0 > 0 is the tail (it waits for them before its first sweep).
// Inside a run every unit but the block's last (s < U - 1) is whole at compile time: both tiles live, no step or store guard, and
// the next unit's samples are 32 floats on.  The block's last unit is peeled, with the general form's guards and its one-tile
// k-loop.  The two cross-ring points are the general form's, statement for statement: same workspace line, nonce flags, fences,
// bounded spin and status word.  The unit's arithmetic is vnet16_common.inc's, called as there: bit-identical decisions.
// COUNT: mvn_vnet_decode_count_f32 (tx != nullptr); the block's bit errors so far are a scalar register across the run.
// (No WRITE_LOGITS, no SURV, no MVN_DIAG_PHASES: those launches stay on vnet16_dealt_kernel.)
// row_time_of / sym_time_of without their selects (which compile to a detour through the exec mask, twice per unit)
constexpr int dealt_row_time(int q) { return 4 * (q ^ (q >> 1)); }
constexpr int dealt_sym_time(int i) { return i ^ ((i >> 1) & 4); }
constexpr bool dealt_times_agree() {
    for (int i = 0; i < 16; ++i)
        if (dealt_sym_time(i) != sym_time_of(i) || dealt_row_time(i >> 2) != row_time_of(i >> 2)) return false;
    return true;
}
static_assert(dealt_times_agree(), "the branch-free forms give row_time_of / sym_time_of");
template <bool COUNT>
__global__ __launch_bounds__(64 * kDealtWaves, 6) void vnet16_dealt_ring1_kernel(
    const float *__restrict__ y, int64_t y_ld, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ final_metric, int B, int T,
    const float *__restrict__ tx, int64_t tx_ld, int K, const unsigned char *__restrict__ row_mask,
    unsigned long long *__restrict__ counters, float *__restrict__ ws, int n_groups, unsigned spin_limit, int skip_publish_ring,
    unsigned long long nonce) {
    constexpr int NT = 2;
    constexpr int S = 16;
    __shared__ Vnet16Image img;
    __shared__ float4 ldsT[kDealtWaves][160];
    __shared__ Vnet16LaneStates lanes;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    const bool odd_w = img.stage(W1, b1, W2, b2, W3, b3);
    lanes.stage();
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<int *>(ws) = 0;  // the status word
    const bool strict = __syncthreads_or(odd_w) != 0;  // the prologue's barrier; workgroup-uniform.  No barrier below.
    const float wmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[0])));
    const float bmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(img.ldsMax[1])));

    // ---- this wave's range of the launch's units (vnet16_dealt_kernel's, at ring = 1) and its runs; all in scalar registers
    const int ring_g = (int)blockIdx.x * kDealtWaves + wave;
    const int n_rings = n_groups * kDealtWaves;
    const int U = (T + kDealtUnit - 1) / kDealtUnit;
    const long long N = (long long)B * U;
    const int lo = (int)(N * ring_g / n_rings), hi = (int)(N * (ring_g + 1) / n_rings);
    const int n = hi - lo;
    const int n_head = hi % U;
    const int n_tail = (lo % U) ? U - lo % U : 0;
    const int has_head = n_head > 0 ? 1 : 0;
    const int n_blocks = (n - n_head - n_tail) / U;
    const int n_runs = has_head + n_blocks + (n_tail > 0 ? 1 : 0);
    const int b_head = hi / U, b_tail = lo / U, b_mid = (lo + n_tail) / U - has_head;  // run r of the whole blocks is block b_mid + r
    auto run_of = [&](int r, int &rb, int &rs0, int &rs1) {  // run r: units rs0 .. rs1 - 1 of block rb
        if (r < has_head) rb = b_head, rs0 = 0, rs1 = n_head;
        else if (r < has_head + n_blocks) rb = b_mid + r, rs0 = 0, rs1 = U;
        else rb = b_tail, rs0 = U - n_tail, rs1 = U;
    };
#if MVN_FN_PRIO
    // the k-loop's priority by the wave's progress (see vnet16_dealt_kernel), its thresholds as execution numbers
#if MVN_DEALT_PMODE == 0
    const int e_p1 = (MVN_DEALT_P1N * n + MVN_DEALT_P1D - 1) / MVN_DEALT_P1D, e_p2 = (MVN_DEALT_P2N * n + MVN_DEALT_P2D - 1) / MVN_DEALT_P2D;
#elif MVN_DEALT_PMODE == 1
    const int e_p1 = n - MVN_DEALT_P1N, e_p2 = n - MVN_DEALT_P2N;
#endif
#endif

    float4 *const tbase = &ldsT[wave][0];
    const int q = lane >> 4;

    int b = 0, s0 = 0, s1 = 0;
    if (n_runs > 0) run_of(0, b, s0, s1);
    float ynext[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int t = s0 * kDealtUnit + 16 * u + sym_time_of(lane & 15);
        ynext[u] = n_runs > 0 ? y[(int64_t)b * y_ld + (t < T ? t : T - 1)] : 0.0f;
    }
    int e = 0;  // the unit's number in the wave's order of execution

    for (int r = 0; r < n_runs; ++r) {
        int bn = b, s0n = s0, s1n = s1;  // the run after this one (after the last: this one again, the prefetch reads what it has read)
        if (r + 1 < n_runs) run_of(r + 1, bn, s0n, s1n);
        // per block, once
        const float *const yrow = y + (int64_t)b * y_ld;
        const float *const y_after = y + (int64_t)bn * y_ld + s0n * kDealtUnit;  // the first samples of the next run ...
        const int tl_after = T - 1 - s0n * kDealtUnit;                             // ... and the last valid offset from there
        float *const decb = dec ? dec + (int64_t)b * dec_ld : nullptr;
        const bool counted = COUNT && (row_mask == nullptr || row_mask[b] != 0);
        const float *const txb = counted ? tx + (int64_t)b * tx_ld : nullptr;
        // what travels along the block, in registers from unit to unit: the path metrics, "the hand-off into this run was
        // abandoned", the bit errors so far
        float m = 0.0f;
        bool bad = false;
        int carry = 0;

        auto unit = [&](auto whole_c, const int s) {
            constexpr bool WHOLE = decltype(whole_c)::value;  // both tiles live, not the block's last unit (s + 1 < U)
            const int t0 = s * kDealtUnit;
#if MVN_FN_PRIO
#if MVN_DEALT_PMODE == 2
            const int c = e % 3;
            if (c == 0) __builtin_amdgcn_s_setprio(2);
            else if (c == 1) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
#else
            if (e < e_p1) __builtin_amdgcn_s_setprio(2);
            else if (e < e_p2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
#endif
#endif
            int lane_k = lane;
            asm volatile("" : "+v"(lane_k));
            const int qk = lane_k >> 4;
            float *const tbw = reinterpret_cast<float *>(tbase) + 4 * (lane_k & 15) + qk;
            float4 *const tbr = tbase + (lane_k & 31);
            const int cunit = lane_k >> 5;
            float yv[NT];
            {  // the next unit's samples are requested now: 32 floats on within the run, else the next run's first
                const bool within = WHOLE && s + 1 < s1;
                const float *const ynx = within ? yrow + t0 + kDealtUnit : y_after;
                const int tl = within ? T - 1 - t0 - kDealtUnit : tl_after;
                const int lt = dealt_sym_time(lane_k & 15);
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    yv[u] = ynext[u];
                    const int tn = lt + 16 * u;
                    ynext[u] = ynx[tn < tl ? tn : tl];
                }
            }
            float ymax = fmaxf(fabsf(yv[0]), fabsf(yv[1]));
            const bool fast = __all(ymax * wmax + bmax <= kFastSigmoidBound);

            f32x4 acc[NT][3];
#pragma unroll
            for (int u = 0; u < NT; ++u)
#pragma unroll
                for (int tau = 0; tau < 3; ++tau) acc[u][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
            float ch[1] = {0.0f};
            const bool one_tile = !WHOLE && t0 + 16 >= T;  // (the block's last unit may end within its first tile)
            if (fast && !one_tile) vnet16_kloop<2, true>([](float d) { return sigmoid_from_neg_fast(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
            else if (!one_tile) vnet16_kloop<2, true>([](float d) { return sigmoid_from_neg(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
            else if (fast) vnet16_kloop<1, true>([](float d) { return sigmoid_from_neg_fast(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);
            else vnet16_kloop<1, true>([](float d) { return sigmoid_from_neg(d); }, img, yv, lane_k, cunit, tbw, tbr, acc, ch);

            float hl[NT];
            vnet16_units4849(img, cunit, tbw, tbr, ch, hl);

#if MVN_FN_PRIO
            __builtin_amdgcn_s_setprio(3);
#endif
            // the tile phase in vnet16_dealt_kernel's three passes
            const int n0 = WHOLE ? 16 : (T - t0 < 16 ? T - t0 : 16);
            const int n1 = WHOLE ? 16 : (T - t0 - 16 < 0 ? 0 : (T - t0 - 16 < 16 ? T - t0 - 16 : 16));
            int lane_t = lane;
            asm volatile("" : "+v"(lane_t));
            const int jt = lane_t & 15, qt = lane_t >> 4;
            const int lane4 = 4 * lane;  // (the one lane-derived value that lives across the k-loop within 80 VGPRs: any other, scratch)
            const int4 ul4 = lanes.ldsLane[lane_t];
            const int ulog[4] = {ul4.x, ul4.y, ul4.z, ul4.w};
            const int row_time = dealt_row_time(qt);
            float cost[NT][4], mrec[NT][4], txv[NT];
            // ---- pass A
            {
                const int row_addr = 4 * (lane_t & 48);
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    const int tdec = t0 + 16 * u + row_time + jt;
                    txv[u] = 0.0f;
                    if (counted && jt < 4 && tdec < K) txv[u] = txb[tdec];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) mrec[u][r4] = 0.0f;
                }
                float logit[NT][4];
                vnet16_tile_pass<NT>(img, tbase, lane_t, acc, hl, logit);
#pragma unroll
                for (int u = 0; u < NT; ++u)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
                        cost[u][r4] = -__int_as_float(__builtin_amdgcn_ds_bpermute(row_addr + 4 * ulog[r4], __float_as_int(logit[u][r4])));
            }
            // ---- pass B: the tail's first unit takes the block's path metrics from the ring that swept its earlier units
            if (s0 > 0 && s == s0) {
                const float *line = ws + (size_t)ring_g * kDealtLineFloats;  // line 1 + (ring_g - 1)
                const unsigned long long *flag = reinterpret_cast<const unsigned long long *>(line) + 9;
                unsigned spins = 0;
                bool ok = true;
                while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nonce) {
                    __builtin_amdgcn_s_sleep(32);
                    if (++spins > spin_limit) {
                        ok = false;
                        break;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                m = line[jt];
                bad = !ok || __builtin_amdgcn_readfirstlane(reinterpret_cast<const int *>(line)[16]) != 0;
                if (!ok && lane_t == 0) __hip_atomic_store(reinterpret_cast<int *>(ws), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // ... the two sweeps ...
            if constexpr (WHOLE) {
                if (!strict) {
                    sweep16_tile<true, false, true>(m, cost[0], mrec[0], 16, lane4, q);
                    sweep16_tile<true, false, true>(m, cost[1], mrec[1], 16, lane4, q);
                } else {
                    sweep16_tile<true, true, true>(m, cost[0], mrec[0], 16, lane4, q);
                    sweep16_tile<true, true, true>(m, cost[1], mrec[1], 16, lane4, q);
                }
            } else if (!strict && n1 == 16) {
                sweep16_tile<true, false, true>(m, cost[0], mrec[0], 16, lane4, q);
                sweep16_tile<true, false, true>(m, cost[1], mrec[1], 16, lane4, q);
            } else if (!strict) {
                sweep16_tile<false, false, true>(m, cost[0], mrec[0], n0, lane4, q);
                if (n1 > 0) sweep16_tile<false, false, true>(m, cost[1], mrec[1], n1, lane4, q);
            } else {
                sweep16_tile<false, true, true>(m, cost[0], mrec[0], n0, lane4, q);
                if (n1 > 0) sweep16_tile<false, true, true>(m, cost[1], mrec[1], n1, lane4, q);
            }
            // ... and, after the head's last unit, on to the ring that sweeps the block's next unit: one line of the workspace
            const bool publish = WHOLE && s + 1 == s1 && s1 < U;
            if (publish) {
                float *line = ws + (size_t)(1 + ring_g) * kDealtLineFloats;
                if (ring_g != skip_publish_ring) {
                    if (lane_t < 16) line[lane_t] = m;
                    if (lane_t == 16) reinterpret_cast<int *>(line)[16] = bad ? 1 : 0;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the line is visible device-wide before the flag
                    unsigned long long nv = nonce;  // (opaque: the VGPR copy of the nonce is made here, not kept -- or spilled -- across the unit loop)
                    asm volatile("" : "+s"(nv));
                    if (lane_t == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(line) + 9, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            // ---- pass C: decisions
            int nerr = 0;
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int nsteps = u == 0 ? n0 : n1;
                const int tdec = t0 + 16 * u + row_time + jt;
                float mydec = strict ? decide4<true>(mrec[u], ulog, jt) : decide4<false>(mrec[u], ulog, jt);
                if (bad) mydec = __int_as_float(0x7fc00000);  // an abandoned hand-off: no decision is claimed
                if (jt < 4 && (WHOLE || row_time + jt < nsteps)) {
                    if (decb) decb[tdec] = mydec;
                    if (counted && tdec < K) nerr += ((long long)mydec != (long long)txv[u]) ? 1 : 0;
                }
            }
            // ---- counting launches: the unit's bit errors join the block's carry
            if constexpr (COUNT) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) nerr += __shfl_xor(nerr, off);
                int total = __builtin_amdgcn_readfirstlane(nerr) + carry;
                if (s0 > 0 && s == s0 && !bad) {  // (after an abandoned wait nothing of that line is waited for again)
                    const int *line = reinterpret_cast<const int *>(ws + (size_t)ring_g * kDealtLineFloats);
                    unsigned spins = 0;
                    while (__hip_atomic_load(reinterpret_cast<const unsigned long long *>(line) + 10, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nonce &&
                           ++spins <= spin_limit)
                        __builtin_amdgcn_s_sleep(32);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    total += __builtin_amdgcn_readfirstlane(line[17]);
                }
                if (publish) {
                    int *line = reinterpret_cast<int *>(ws + (size_t)(1 + ring_g) * kDealtLineFloats);
                    if (ring_g != skip_publish_ring) {
                        if (lane == 0) line[17] = total;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                        unsigned long long nv = nonce;
                        asm volatile("" : "+s"(nv));
                        if (lane == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(line) + 10, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else if (WHOLE) {
                    carry = total;
                } else if (counted && total != 0 && lane == 0) {  // the block ends here: two global atomics per block in error
                    atomicAdd(&counters[0], (unsigned long long)total);
                    atomicAdd(&counters[2], 1ull);
                }
            }
            if (!WHOLE && final_metric) {  // (the lane id is made opaque: nothing lane-derived is hoisted out of the unit loop)
                int lane_f = lane;
                asm volatile("" : "+v"(lane_f));
                if (lane_f < 16) final_metric[(int64_t)b * S + logical_state(lane_f, T & 3)] = m;
            }
            ++e;
        };

        const int s_whole = s1 == U ? U - 1 : s1;  // the run's whole units: s0 .. s_whole - 1
        for (int s = s0; s < s_whole; ++s) unit(std::true_type{}, s);
        if (s1 == U) unit(std::false_type{}, U - 1);  // the block's last unit
        b = bn, s0 = s0n, s1 = s1n;
    }
}
