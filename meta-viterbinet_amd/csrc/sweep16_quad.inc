// sweep16_quad.inc -- 16 blocks per wavefront variant of the cost-streaming 16-state sweep (mvn_acs_sweep_f32 and
// the sweep of the two-kernel ViterbiNet route), included by mvn_hip.hip after sweep16_lds.inc.
//
// sweep16_lds_kernel keeps one state per lane (4 blocks per wave) and spends ~14 VALU instructions per trellis step
// on them, 3.5 per block-step: at BASELINE's 10 000 blocks (2.4 waves per SIMD) that instruction stream, not HBM, is
// what the launch waits for.  Here a block's 16 path metrics live in 4 lanes x 4 VGPRs (lane quad = block, so a
// wave owns 16 blocks) and the in-place ACS recurrence (trellis_utils.py:16-30) uses one partner operation per
// bit of the slot index X = l | r << 2 (l = lane & 3, r = register), cyclically with phase rho = t % 4:
//     rho 0 : lane ^ 1  (quad_perm [1,0,3,2])      one v_min_f32_dpp per register
//     rho 1 : lane ^ 2  (quad_perm [2,3,0,1])      one v_min_f32_dpp per register
//     rho 2 : register ^ 1                          two in-lane v_min_f32
//     rho 3 : register ^ 2                          two in-lane v_min_f32
// The logical state of slot X at phase rho is rotr4(X, rho).  ~20 VALU instructions per step serve 16 blocks
// (1.25 per block-step).  Decisions: as in the other in-place kernels, the metrics before a stage are equal in the
// pairs joined by the previous stage's operation (logical states s and s+8), so reducing over the other three
// operations yields the block minimum and the minimal tying index up to +8 -- the same least-significant bit.
//
// Costs arrive by LDS-DMA exactly as in sweep16_lds_kernel, one 1-KB piece = 16 steps of one block, 16 pieces per
// chunk, ring of kQuadRing chunks per wave (one wave per workgroup, 3 x 16.25 KB of LDS, 3 workgroups per CU).
// Block images are padded by 16 B so the quads' reads spread over the banks at rho 0.
// vmcnt bookkeeping: per chunk 16 DMA pieces (G) and NS decision stores (S; 1 if rows are 16-B aligned, else 4);
// when chunk c is consumed the younger operations are S(c-R), then (R-1) x {G, S} -> vmcnt(16 (R-1) + R NS), fewer
// stores in the first R chunks.
constexpr int kQuadRing = 3;
constexpr int kQuadBlockFloats = 16 * 16 + 4;
constexpr int kQuadChunkFloats = 16 * kQuadBlockFloats;

__host__ __device__ constexpr int quad_logical(int l, int r, int rho) {
    return (((l | (r << 2)) | ((l | (r << 2)) << 4)) >> rho) & 15;
}

// in-lane minima as plain VALU instructions (fminf() would first canonicalise operands that come out of inline asm)
__device__ __forceinline__ float vmin2(float a, float b) {
    float r;
    asm("v_min_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// torch.min over the two candidates of a state: NaN when either is NaN, else the smaller (oracle: min2_torch; the value is
// symmetric in its operands, and every caller discards the index)
__device__ __forceinline__ float min2_strict(float a, float b) {
    const float r = vmin2(a, b);
    return (a != a || b != b) ? __int_as_float(0x7fc00000) : r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// four registers against their lane partners, in place, behind ONE pair of hazard wait states
#define MVN_MIN4_DPP(NAME, CTRL_STR)                                                                       \
    __device__ __forceinline__ void NAME(float (&a)[4]) {                                                  \
        asm("s_nop 1\n\t"                                                                                  \
            "v_min_f32_dpp %0, %0, %0 " CTRL_STR " row_mask:0xf bank_mask:0xf\n\t"                         \
            "v_min_f32_dpp %1, %1, %1 " CTRL_STR " row_mask:0xf bank_mask:0xf\n\t"                         \
            "v_min_f32_dpp %2, %2, %2 " CTRL_STR " row_mask:0xf bank_mask:0xf\n\t"                         \
            "v_min_f32_dpp %3, %3, %3 " CTRL_STR " row_mask:0xf bank_mask:0xf"                             \
            : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));                                             \
    }
MVN_MIN4_DPP(min4_xor1, "quad_perm:[1,0,3,2]")
MVN_MIN4_DPP(min4_xor2, "quad_perm:[2,3,0,1]")
#undef MVN_MIN4_DPP

// LSB of the first minimal logical state before a phase-RHO stage; U[r] = logical state of (lane, r) at RHO
template <int RHO>
__device__ __forceinline__ int quad_decide(const float (&m)[4], const int (&U)[4]) {
    constexpr int PREV = (RHO + 3) & 3;
    float v;
    if (PREV == 2) v = vmin2(m[0], m[2]);       // registers r and r^1 are equal
    else if (PREV == 3) v = vmin2(m[0], m[1]);  // registers r and r^2 are equal
    else v = vmin3(m[0], m[1], vmin2(m[2], m[3]));
    if (PREV != 0) v = min_xor1(v);
    if (PREV != 1) v = min_xor2(v);
    // U[r] grows with r at every phase, so the lane's first minimal slot is found by a select chain from the top
    int c = 16;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
        if (PREV == 2 && (r & 1)) continue;
        if (PREV == 3 && (r & 2)) continue;
        c = m[r] == v ? U[r] : c;
    }
    if (PREV != 0) c = min(c, dpp_i32<MVN_DPP_XOR1>(c));
    if (PREV != 1) c = min(c, dpp_i32<MVN_DPP_XOR2>(c));
    return c & 1;
}

template <int RHO, int MODE>
__device__ __forceinline__ void quad_stage(float (&m)[4], const float (&c)[4]) {
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = MODE == MODE_NEGLOGIT ? m[r] - c[r] : m[r] + c[r];
    if (RHO == 0) {
        min4_xor1(a);
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = a[r];
    } else if (RHO == 1) {
        min4_xor2(a);
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = a[r];
    } else if (RHO == 2) {
        m[0] = m[1] = vmin2(a[0], a[1]);
        m[2] = m[3] = vmin2(a[2], a[3]);
    } else {
        m[0] = m[2] = vmin2(a[0], a[2]);
        m[1] = m[3] = vmin2(a[1], a[3]);
    }
}

// the same two with torch.min's / torch.argmin's NaN rule (taken from the first odd cost on, odd_cost() in vnet16_common.inc): the
// pairs joined by the previous stage still hold equal metrics (the strict stage writes one value to both partners)
template <int RHO>
__device__ __forceinline__ int quad_decide_strict(const float (&m)[4], const int (&U)[4]) {
    constexpr int PREV = (RHO + 3) & 3;
    int k[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) k[r] = strict_key(m[r]);
    int v;
    if (PREV == 2) v = min(k[0], k[2]);
    else if (PREV == 3) v = min(k[0], k[1]);
    else v = min(min(k[0], k[1]), min(k[2], k[3]));
    if (PREV != 0) v = min(v, dpp_i32<MVN_DPP_XOR1>(v));
    if (PREV != 1) v = min(v, dpp_i32<MVN_DPP_XOR2>(v));
    int c = 16;
#pragma unroll
    for (int r = 3; r >= 0; --r) {
        if (PREV == 2 && (r & 1)) continue;
        if (PREV == 3 && (r & 2)) continue;
        c = k[r] == v ? U[r] : c;
    }
    if (PREV != 0) c = min(c, dpp_i32<MVN_DPP_XOR1>(c));
    if (PREV != 1) c = min(c, dpp_i32<MVN_DPP_XOR2>(c));
    return c & 1;
}
template <int RHO, int MODE>
__device__ __forceinline__ void quad_stage_strict(float (&m)[4], const float (&c)[4]) {
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = MODE == MODE_NEGLOGIT ? m[r] - c[r] : m[r] + c[r];
    if (RHO == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = min2_strict(a[r], dpp_f32<MVN_DPP_XOR1>(a[r]));
    } else if (RHO == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = min2_strict(a[r], dpp_f32<MVN_DPP_XOR2>(a[r]));
    } else if (RHO == 2) {
        m[0] = m[1] = min2_strict(a[0], a[1]);
        m[2] = m[3] = min2_strict(a[2], a[3]);
    } else {
        m[0] = m[2] = min2_strict(a[0], a[2]);
        m[1] = m[3] = min2_strict(a[1], a[3]);
    }
}

// ---- survivors (SURVEY 8, row "traceback pointers": what acs_block returns and every caller drops, trellis_utils.py:30).
// A stage joins the slot whose coordinate bit RHO is 0 -- it holds the EVEN predecessor p0 = 2 s' of new states s' and s' + 8 --
// with its partner (p1 = 2 s' + 1); torch.min's index is j = 1 iff the odd candidate is strictly smaller (NaN: the first NaN).
// Without odd costs (the kernel's plain form) that is "the minimum is not the even candidate": one compare per pair, taken where
// the even candidate lives; K (per lane and register, 0 where the slot holds an odd predecessor) are the two bits of s' and s' + 8 in
// the step's 16-bit survivor word.  With odd costs about (ST): torch's rule written out.  Returns the word, OR-ed over the quad.
__device__ __forceinline__ float vmin_dpp_xor1(float a) {
    float r;
    asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(a));
    return r;
}
__device__ __forceinline__ float vmin_dpp_xor2(float a) {
    float r;
    asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(a));
    return r;
}
template <int RHO, int MODE, bool ST>
__device__ __forceinline__ unsigned quad_stage_surv(float (&m)[4], const float (&c)[4], const unsigned (&K)[4]) {
    float a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = MODE == MODE_NEGLOGIT ? m[r] - c[r] : m[r] + c[r];
    unsigned word = 0;
    auto join = [&](float even, float odd, unsigned k) {  // -> the stage's value; adds k to the word when the odd candidate survives
        const float mn = ST ? min2_strict(even, odd) : vmin2(even, odd);
        const bool j = ST ? (even == even && !(odd >= even)) : (mn != even);
        word |= j ? k : 0u;
        return mn;
    };
    if (RHO < 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (ST) {
                m[r] = join(a[r], RHO == 0 ? dpp_f32<MVN_DPP_XOR1>(a[r]) : dpp_f32<MVN_DPP_XOR2>(a[r]), K[r]);
            } else {  // (the lanes of odd predecessors compare against their own candidate: K = 0 there)
                const float mn = RHO == 0 ? vmin_dpp_xor1(a[r]) : vmin_dpp_xor2(a[r]);
                word |= mn != a[r] ? K[r] : 0u;
                m[r] = mn;
            }
        }
    } else if (RHO == 2) {
        m[0] = m[1] = join(a[0], a[1], K[0]);
        m[2] = m[3] = join(a[2], a[3], K[1]);
    } else {
        m[0] = m[2] = join(a[0], a[2], K[0]);
        m[1] = m[3] = join(a[1], a[3], K[1]);
    }
    word |= (unsigned)dpp_i32<MVN_DPP_XOR1>((int)word);
    word |= (unsigned)dpp_i32<MVN_DPP_XOR2>((int)word);
    return word;
}

// SURV (round 5): also stores the survivors, surv[b][t] = 16 bits (bit s = j of new state s), one 8-byte store per lane and chunk
// (4 steps; a block's 32 bytes per chunk are contiguous).  The launcher takes this form only for 16-byte-aligned decision rows,
// T % 4 == 0 and 8-byte-aligned survivor rows (otherwise: sweep_surv_kernel).
template <int MODE, bool VEC4, bool SURV = false>
__global__ __launch_bounds__(64) void sweep16_quad_kernel(const float *__restrict__ src, float *__restrict__ dec,
                                                          int64_t dec_ld, float *__restrict__ final_metric, int64_t B,
                                                          int T, int base, int extra, unsigned char *__restrict__ surv) {
    constexpr int S = 16;
    static_assert(!SURV || VEC4, "survivors: the vector-store form");
    constexpr int NS = (VEC4 ? 1 : 4) + (SURV ? 1 : 0);  // decision (and survivor) stores per full chunk
    static_assert(16 * (kQuadRing - 1) + NS * kQuadRing <= 63, "vmcnt is a 6-bit counter");
    __shared__ __attribute__((aligned(16))) float lds[kQuadRing][kQuadChunkFloats];
    const int lane = threadIdx.x;
    const int l = lane & 3;
    const int g = lane >> 2;
    // this wave's blocks: `base` of them (16, or fewer when the launcher evens the blocks out over one round of waves), the first
    // `extra` waves one more; b0 < B by the grid size
    const int64_t b0 = (int64_t)blockIdx.x * base + ((int)blockIdx.x < extra ? (int)blockIdx.x : extra);
    const int mine = base + ((int)blockIdx.x < extra ? 1 : 0);
    const int nvalid = B - b0 < mine ? (int)(B - b0) : mine;
    const int64_t b = b0 + g;
    const bool active = g < nvalid;

    int U[4][4];  // logical state of slot (lane, r) at phase rho
#pragma unroll
    for (int rho = 0; rho < 4; ++rho)
#pragma unroll
        for (int r = 0; r < 4; ++r) U[rho][r] = quad_logical(l, r, rho);
    // per-lane LDS read bases (floats): block image + the lane-dependent part of the logical state; the register
    // part is a compile-time offset: rho 0: 4r, rho 1: 2r, rho 2: r, rho 3: (r >> 1) + 8 (r & 1)
    const int rb[4] = {g * kQuadBlockFloats + l, g * kQuadBlockFloats + (l >> 1) + 8 * (l & 1),
                       g * kQuadBlockFloats + 4 * l, g * kQuadBlockFloats + 2 * l};

    const int nchunks = (T + 15) / 16;
    // row pointers of the 16 blocks (uniform, loop-invariant: SGPR base + per-lane VGPR offset addressing)
    const float *rowp[16];
#pragma unroll
    for (int blk = 0; blk < 16; ++blk) {
        const int bi = blk < nvalid ? blk : nvalid - 1;  // past the batch: re-read the last block, never stored
        rowp[blk] = src + (b0 + bi) * ((int64_t)T * S);
    }
    auto issue_chunk = [&](int c, int slot) {
        int step = 16 * c + g;
        if (step >= T) step = T - 1;  // partial last chunk: re-read valid data, never used
        const unsigned voff = (unsigned)(step * S + 4 * l);
#pragma unroll
        for (int blk = 0; blk < 16; ++blk)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(rowp[blk] + voff),
                                             (__attribute__((address_space(3))) void *)&lds[slot][blk * kQuadBlockFloats],
                                             16, 0, MVN_SWEEP_GLDS_AUX);
    };

    // survivor-word bits of the slots that hold an even predecessor at phase rho (quad_stage_surv): rho 0 / 1 per register,
    // rho 2: pairs (0, 1) and (2, 3), rho 3: pairs (0, 2) and (1, 3); the new state is the slot's logical state at phase rho + 1
    unsigned KS[4][4] = {};
    if constexpr (SURV) {
        auto pair_bits = [](int s_new) { return 0x0101u << (s_new & 7); };
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            KS[0][r] = (l & 1) ? 0u : pair_bits(U[1][r]);
            KS[1][r] = (l & 2) ? 0u : pair_bits(U[2][r]);
        }
        KS[2][0] = pair_bits(U[3][0]), KS[2][1] = pair_bits(U[3][2]);
        KS[3][0] = pair_bits(U[0][0]), KS[3][1] = pair_bits(U[0][1]);
    }
    unsigned char *const srow = SURV ? surv + ((size_t)b * T) * 2 + 8 * l : nullptr;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float cur[16][4];
    auto consume_chunk = [&](int slot) {
        const float *img = &lds[slot][0];
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[i][r] = img[rb[i & 3] + i * 16 + quad_logical(0, r, i & 3)];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot may be refilled from here on
    };
    float *const drow = dec + b * dec_ld;
    bool strict = false;  // wave-uniform, sticky: an odd cost (NaN, infinite, huge) has come by
    auto process_chunk = [&](int c, auto full, auto strict_c) {
        constexpr bool ST = decltype(strict_c)::value;
        const int t0 = 16 * c;
        unsigned bits = 0;  // bit i = decision of step t0 + i (the same in the 4 lanes of a block)
        unsigned svw[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // SURV: the chunk's 16 survivor words, two per register (the same in the 4 lanes)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (decltype(full)::value || t0 + i < T) {  // wave-uniform
                const int rho = i & 3;
                int bit;
                if (ST)
                    bit = rho == 0 ? quad_decide_strict<0>(m, U[0]) : rho == 1 ? quad_decide_strict<1>(m, U[1])
                        : rho == 2 ? quad_decide_strict<2>(m, U[2]) : quad_decide_strict<3>(m, U[3]);
                else
                    bit = rho == 0 ? quad_decide<0>(m, U[0]) : rho == 1 ? quad_decide<1>(m, U[1])
                        : rho == 2 ? quad_decide<2>(m, U[2]) : quad_decide<3>(m, U[3]);
                bits |= (unsigned)bit << i;
                if constexpr (SURV) {
                    const unsigned w = rho == 0 ? quad_stage_surv<0, MODE, ST>(m, cur[i], KS[0]) : rho == 1 ? quad_stage_surv<1, MODE, ST>(m, cur[i], KS[1])
                                     : rho == 2 ? quad_stage_surv<2, MODE, ST>(m, cur[i], KS[2]) : quad_stage_surv<3, MODE, ST>(m, cur[i], KS[3]);
                    svw[i >> 1] |= w << (16 * (i & 1));
                } else if (ST) {
                    if (rho == 0) quad_stage_strict<0, MODE>(m, cur[i]);
                    else if (rho == 1) quad_stage_strict<1, MODE>(m, cur[i]);
                    else if (rho == 2) quad_stage_strict<2, MODE>(m, cur[i]);
                    else quad_stage_strict<3, MODE>(m, cur[i]);
                } else {
                    if (rho == 0) quad_stage<0, MODE>(m, cur[i]);
                    else if (rho == 1) quad_stage<1, MODE>(m, cur[i]);
                    else if (rho == 2) quad_stage<2, MODE>(m, cur[i]);
                    else quad_stage<3, MODE>(m, cur[i]);
                }
            }
        }
        if constexpr (SURV) {  // lane l of the quad: steps 4 l .. 4 l + 3 = 8 bytes (whole chunks; a word's last steps one by one)
            const unsigned w0 = l == 0 ? svw[0] : l == 1 ? svw[2] : l == 2 ? svw[4] : svw[6];
            const unsigned w1 = l == 0 ? svw[1] : l == 1 ? svw[3] : l == 2 ? svw[5] : svw[7];
            unsigned char *sp = srow + 2 * t0;
            if (decltype(full)::value) {
                if (active) *reinterpret_cast<uint2 *>(sp) = make_uint2(w0, w1);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (active && t0 + 4 * l + e < T)
                        reinterpret_cast<unsigned short *>(sp)[e] = (unsigned short)((e < 2 ? w0 : w1) >> (16 * (e & 1)));
            }
        }
        // 64 B of decisions per block and chunk.  Batching 2 or 4 chunks per store (128/256 B per row) and
        // nontemporal stores were measured: no gain / a loss (DESIGN.md 5.2b).
        float *dp = drow + t0;
        if (VEC4 && decltype(full)::value) {
            const unsigned q = bits >> (4 * l);
            const float4 o = {(float)(q & 1u), (float)((q >> 1) & 1u), (float)((q >> 2) & 1u), (float)((q >> 3) & 1u)};
            if (active) *reinterpret_cast<float4 *>(dp + 4 * l) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // the quad writes 4 consecutive steps per store
                const int i = 4 * e + l;
                if (active && (decltype(full)::value || t0 + i < T)) dp[i] = (float)((bits >> i) & 1u);
            }
        }
    };

    // prologue: fill the ring
#pragma unroll
    for (int k = 0; k < kQuadRing; ++k)
        if (k < nchunks) issue_chunk(k, k);

    for (int cb = 0; cb < nchunks; cb += kQuadRing) {
#pragma unroll
        for (int k = 0; k < kQuadRing; ++k) {
            const int c = cb + k;
            if (c < nchunks) {  // wave-uniform
                const bool more = c + kQuadRing < nchunks;
                if (!more || strict) {
                    wait_vmcnt<0>();  // draining: nothing younger is guaranteed to be in flight (strict: a chunk's stores were issued twice)
                } else {
                    // younger than G(c): the (R-1) chunks queued behind it and the stores of up to R earlier chunks
                    if (c == 0) wait_vmcnt<16 * (kQuadRing - 1)>();
                    else if (c == 1) wait_vmcnt<16 * (kQuadRing - 1) + NS>();
                    else if (c == 2) wait_vmcnt<16 * (kQuadRing - 1) + 2 * NS>();
                    else wait_vmcnt<16 * (kQuadRing - 1) + 3 * NS>();
                }
                consume_chunk(k);
                if (more) issue_chunk(c + kQuadRing, k);
                // Every cost is tested for oddness (any_odd_cost, vnet16_common.inc).  A lone wave per SIMD pays every extra
                // instruction's latency, so on whole chunks the test is computed BESIDE the recurrence it does not depend on (one
                // basic block: the scheduler interleaves the two) and a chunk that turns out to hold an odd cost is processed
                // again from the saved metrics with the NaN-propagating forms; its decisions are stored over the first ones.
                // (costs of lanes past the batch are re-reads of a valid block: no false alarm, and harmless if one)
                if (strict) {
                    process_chunk(c, std::false_type{}, std::true_type{});
                } else if (16 * c + 16 <= T) {
                    const float m0[4] = {m[0], m[1], m[2], m[3]};
                    const bool odd = any_odd_cost(reinterpret_cast<const float(&)[64]>(cur));
                    process_chunk(c, std::true_type{}, std::false_type{});
                    if (__any(odd)) {
                        strict = true;
#pragma unroll
                        for (int r = 0; r < 4; ++r) m[r] = m0[r];
                        wait_vmcnt<0>();  // (the stores above have left before the same addresses are written again)
                        process_chunk(c, std::false_type{}, std::true_type{});
                    }
                } else {
                    strict = __any(any_odd_cost(reinterpret_cast<const float(&)[64]>(cur))) != 0;
                    if (strict) process_chunk(c, std::false_type{}, std::true_type{});
                    else process_chunk(c, std::false_type{}, std::false_type{});
                }
            }
        }
    }
    if (active && final_metric) {
        const int rho = T & 3;
#pragma unroll
        for (int r = 0; r < 4; ++r) final_metric[b * S + quad_logical(l, r, rho)] = m[r];
    }
}

// When is this variant the default?  Its 48.75 KB of LDS per wave allow 3 waves per CU, so the launch runs in rounds
// of 3 x CUs waves (768 on MI355X = 12 288 blocks) and a thinly filled last round costs as much as a full one.
// Measured against sweep16_lds_kernel at T = 1000 (tools/time_sweep.py, profiles/r01_time_acs_sweep_variants.txt):
// +3..13 % at 8 000-12 000 blocks and +2..16 % at 24 000 (last round 65-98 % full), -3..-6 % at 16 000, 30 000, 40 000
// and 100 000 (last round 14-44 % full).  Rule: last round at least 60 % full, and not more than 4 rounds.
inline bool sweep16_quad_preferred(int64_t B) {
    const int n_cu = current_device_cus();  // (atomic, per device: mvn_hip.hip)
    const int slots = 3 * (n_cu > 0 ? n_cu : 256);
    const int64_t waves = (B + 15) / 16;
    const int64_t rounds = (waves + slots - 1) / slots;
    const int64_t last = waves - (rounds - 1) * slots;
    return rounds <= 4 && 10 * last >= 6 * slots;
}

// Blocks per wave.  A launch that fits ONE round of waves (3 per CU) but does not fill it whole CUs at a time leaves some CUs with
// one 16-block wave more than the others (10 000 blocks: 625 waves, 113 CUs stream 48 blocks while 143 stream 32), and the launch
// lasts as long as the fullest CU.  Such a launch is dealt evenly instead: k waves per CU for the smallest k in 1..3 that keeps a
// wave within 16 blocks, `base` = B / (k CUs) blocks each and one more for the first `extra` (10 000 blocks: k = 3, 768 waves of 13,
// sixteen of them 14; 8 000: k = 2, 512 waves of 15 or 16; measured at 10 000 blocks: 0.132-0.140 -> 0.132-0.134 ms).  A wave's unused lane quads idle -- but a wave costs its instructions
// whatever it carries, so k is not raised beyond need (three thin waves per CU were measured slower than two full ones).
// Everything else runs 16 blocks per wave.
inline void sweep16_quad_deal(int64_t B, int &base, int &extra, int64_t &grid) {
    const int n_cu = current_device_cus();
    const int cus = n_cu > 0 ? n_cu : 256;
    base = 16, extra = 0, grid = (B + 15) / 16;
    const int64_t k = (B + (int64_t)16 * cus - 1) / ((int64_t)16 * cus);  // waves per CU needed at 16 blocks per wave
    if (k >= 1 && k <= 3 && B >= (int64_t)12 * k * cus) {  // (waves at least three quarters full: below, 16-block waves were faster)
        const int64_t waves = k * cus;
        base = (int)(B / waves);
        extra = (int)(B - (int64_t)base * waves);
        grid = waves;
    }
}

// the survivor form's conditions (else the generic sweep_surv_kernel runs): LDS-DMA of the costs and vector stores throughout
inline bool sweep16_quad_surv_serves(const float *src, const float *dec, int64_t dec_ld, const unsigned char *surv, int T) {
    return (reinterpret_cast<uintptr_t>(src) % 16) == 0 && (dec_ld % 4) == 0 && (reinterpret_cast<uintptr_t>(dec) % 16) == 0 &&
           (T % 4) == 0 && (reinterpret_cast<uintptr_t>(surv) % 8) == 0;
}
template <int MODE>  // MODE_COST: materialised costs; MODE_NEGLOGIT: the ViterbiNet logits (branch cost = -logit)
int launch_sweep16_quad_surv(const float *src, float *dec, int64_t dec_ld, float *final_metric, unsigned char *surv, int64_t B, int T,
                             hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    int base, extra;
    int64_t grid;
    sweep16_quad_deal(B, base, extra, grid);
    hipLaunchKernelGGL((sweep16_quad_kernel<MODE, true, true>), dim3((unsigned)grid), dim3(64), 0, st, src, dec, dec_ld, final_metric,
                       B, T, base, extra, surv);
    return (int)hipGetLastError();
}

template <int MODE>
int launch_sweep16_quad(const float *src, float *dec, int64_t dec_ld, float *final_metric, int64_t B, int T,
                        hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    int base, extra;
    int64_t grid;
    sweep16_quad_deal(B, base, extra, grid);
    const bool vec4 = (dec_ld % 4) == 0 && (reinterpret_cast<uintptr_t>(dec) % 16) == 0;
    if (vec4)
        hipLaunchKernelGGL((sweep16_quad_kernel<MODE, true>), dim3((unsigned)grid), dim3(64), 0, st, src, dec, dec_ld,
                           final_metric, B, T, base, extra, (unsigned char *)nullptr);
    else
        hipLaunchKernelGGL((sweep16_quad_kernel<MODE, false>), dim3((unsigned)grid), dim3(64), 0, st, src, dec, dec_ld,
                           final_metric, B, T, base, extra, (unsigned char *)nullptr);
    return (int)hipGetLastError();
}
