// vnet_fused_ip.inc -- the ViterbiNet detector for every S = 4 << LB other than 16 in ONE kernel: the likelihood MLP fused into
// the trellis sweep, logits never in HBM (8 B/symbol of traffic instead of 8 S + 8).  Included by mvn_hip.hip after
// sweep_inplace.inc.
//
// VNETDetector.forward(y, 'val') (python_code/detectors/VNET/vnet_detector.py:35-61) takes any n_states; rounds 1-3 fused it at
// 16 states only (vnet16_fusedn.inc) and sent every other S through mlp_kernel -> [B, T, S] logits in HBM -> sweep_inplace_kernel.
// Here a wavefront owns two blocks (one at S = 256) for all T symbols, in sweep_inplace_kernel's layout, and alternates per chunk
// of CS trellis steps (32 symbols: 2 blocks x 16 steps) between
//   * the MLP of the chunk's symbols, two 16-symbol tiles in flight.  S <= 128 (round 5): vnet16_fusedn.inc's k-loop -- layer 1 +
//     sigmoid straight into the MFMA B operand, three row tiles of v_mfma_f32_16x16x4_f32 for hidden-2 units 0..47 with W2 read
//     from LDS, units 48 / 49 as k-ordered fmaf chains on the vector ALU through a wave-private LDS image, bias / ReLU / the (q, r)
//     transposes through the same image, layer 3 with W3 from LDS: 150 instead of 200 MFMAs per 32 symbols, and every per-lane
//     constant fetched from LDS or recomputed from an opaque lane id where it is used, so that the kernel needs 81-95 VGPRs (round
//     4: 124-168) and the waves per SIMD are set by the LDS images.  S = 256: mlp_kernel's tile (four row tiles, W2's
//     operands as float4s).  Either way the same k-ordered fmaf chains: the logits are bit for bit mlp_kernel's (= the
//     reference's).  They are written into the wave's LDS chunk image in the layout sweep_inplace_kernel's DMA would have produced;
//   * sweep_inplace_kernel's consumer: the in-place recurrence of va_inplace.inc on 2^LB lanes x 4 VGPRs per block, each lane
//     reading the 4 costs of its current logical states from the image (their numbers per phase come from a small LDS table).
//     A whole chunk (S <= 64, plain minimum) runs unrolled, one copy per starting phase: phases, image rows and decision bits are
//     immediates (~15-30 instructions per step, no branch); the last chunk of a word and the NaN-propagating form take a step
//     loop that switches over the LB + 2 compile-time stage bodies.  A chunk's decisions are 16 bits of a register, one LDS word
//     per block and chunk, expanded to floats by the flush.
// No barrier after the prologue, no traffic between waves.
// torch.min's NaN rule (trellis_utils.py:30): the stage is v_min_f32 (minNum) like every in-place kernel, which differs from
// torch.min only when SOME BUT NOT ALL of a symbol's branch costs are NaN; that takes a non-finite or absurdly large weight, which
// the prologue looks for once (as vnet16_fusedn does); the launch then runs the NaN-propagating forms of the stage and of the
// decision below (first NaN, else first minimum) -- no guard launch, there are no logits in HBM to re-decode from.
// Workgroups are FOUR waves (one per SIMD: a workgroup of 10 or 6 waves loads the SIMDs 3/3/2/2 and runs 20 % slower than one of
// 8 or 12, tools/ab_ip.py) and as many per CU as the LDS holds: five at S = 4 / 8 (27-30 KB each), three at 32, two at 64 (one of
// twelve waves at 128) --
// 10 000 blocks are 1 250 workgroups = ONE round of the chip at 4 / 8 states.  Measured at 10 000 x 1000 (round 4 -> round 5):
// S = 4: 1.97 -> 1.55 ms, 8: 2.13 -> 1.44, 32: 2.30 -> 1.78, 64: 2.99 -> 2.46 (profiles/r05_time_vnet_states.txt).
template <int LB>
constexpr bool vnet_ip_k3() { return LB <= 5; }
// S = 128: the chunk image holds HALF a chunk -- tile u is steps 8 u .. 8 u + 7 of both blocks, and layer 3 + sweep run per tile --
// so that it is 8 KB per wave instead of 16 and twelve waves (three per SIMD) share a CU where round 4's kernel had four
template <int LB>
constexpr int vnet_ip_image_steps() { return LB == 5 ? 8 : 16 * (LB <= 5 ? 2 : 1) / ((64 >> LB) >= 2 ? 2 : 1); }
#ifndef MVN_IP_WAVES
#define MVN_IP_WAVES(LB) ((LB) == 5 ? 12 : 4)
#endif
#ifndef MVN_IP_PRIO
#define MVN_IP_PRIO 1  // wave-priority rules of the main loop (0 = off, for A/B runs)
#endif
#ifndef MVN_IP_UNROLL
#define MVN_IP_UNROLL 1  // whole chunks' trellis steps unrolled per starting phase (0: the step loop only, for A/B runs)
#endif
#ifndef MVN_IP_ALIAS
#define MVN_IP_ALIAS(LB) ((LB) <= 1 || (LB) == 5)
#endif
#ifndef MVN_IP_WGS
#define MVN_IP_WGS(LB) ((LB) <= 1 ? 5 : (LB) == 3 ? 3 : (LB) == 4 ? 2 : 1)
#endif
template <int LB>
constexpr int vnet_ip_waves() { return MVN_IP_WAVES(LB); }
template <int LB>
constexpr int vnet_ip_wgs() { return MVN_IP_WGS(LB); }  // workgroups per CU the kernel is built for

template <int LB>
constexpr int vnet_ip_blocks() { return (64 >> LB) >= 2 ? 2 : 1; }  // blocks per wave: 2 (1 at S = 256) -- round 4 measured 4 or 1: 10-15 % slower
template <int LB>
constexpr int vnet_ip_tiles() { return LB <= 5 ? 2 : 1; }  // 16-symbol MLP tiles a wave keeps in flight (two independent sigmoid chains)
template <int LB>
constexpr int vnet_ip_chunk() {  // trellis steps per chunk: blocks x CS = 16 symbols per tile in flight
    return 16 * vnet_ip_tiles<LB>() / vnet_ip_blocks<LB>();
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a compile-time constant
template <class F, int... J>
__device__ __forceinline__ void static_for_each(F &&f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}

// (the NaN-propagating stage and decision -- va_ip_key, va_ip_acs_strict, va_ip_decide_strict -- live in va_inplace.inc: the
// sweeps over materialised costs take them too)
template <int LB>
__global__ __launch_bounds__(64 * vnet_ip_waves<LB>(), (vnet_ip_waves<LB>() * vnet_ip_wgs<LB>() + 3) / 4) void vnet_fused_ip_kernel(
    const float *__restrict__ y, int64_t y_ld, const float *__restrict__ W1, const float *__restrict__ b1,
    const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3, const float *__restrict__ b3,
    float *__restrict__ dec, int64_t dec_ld, float *__restrict__ final_metric, int64_t B, int T, int aligned) {
    constexpr int N = LB + 2, NL = 1 << LB, S = 4 << LB, CS = vnet_ip_chunk<LB>(), kVfWaves = vnet_ip_waves<LB>();
    // blocks of a wave: the sweep's layout has room for 64 >> LB, but the MLP -- the work -- parallelises over WAVES here, so a
    // wave takes at most 4 blocks (one 16-symbol tile per 4-step chunk) and leaves the other lanes of its sweep idle (S < 64)
    constexpr int BPW = vnet_ip_blocks<LB>();
    constexpr int HS = vnet_ip_image_steps<LB>();             // steps of a block the chunk image holds: CS, or CS / 2 (S = 128)
    constexpr bool HALF = HS != CS;
    static_assert(HS == CS || (2 * HS == CS && BPW * HS == 16), "a half chunk is one tile: HS steps of every block");
    constexpr int IMG = HS * S;                               // floats of one block's HS steps
    constexpr int NS = BPW * CS >= 256 ? BPW * CS / 256 : 1;  // float4 decision stores per lane and chunk
    constexpr int CF = BPW * IMG + 4 * ((BPW * IMG + 255) / 256) + 4;  // chunk image: BPW blocks of CS x S costs, 4 floats of padding per 256
    constexpr int NT3 = (S + 15) / 16;                        // 16-state tiles of the output layer
    constexpr int NTILE = BPW * CS / 16;                      // 16-symbol MLP tiles per chunk
    static_assert(BPW * CS % 16 == 0 && CS % 4 == 0, "whole tiles, float4 decision rows");
    constexpr bool K3 = vnet_ip_k3<LB>();
    __shared__ float ldsA3[NT3 * kK3Steps * 64];
    __shared__ float ldsB3[NT3 * 16];
    __shared__ float4 ldsA2[K3 ? 1 : kK2Steps * 64];  // (i, lane) -> W2[{0, 16, 32, 48} + (lane & 15)][4 i + (lane >> 4)] (units >= 50: 0)
    __shared__ float2 ldsWB[kK2Steps * 4];   // (i, q) -> {-w1, -b1}[4 i + q]
    // K3 (vnet16_fusedn.inc's images): W2's units 0..47 as A operands, units 48 / 49 as the chains' weights, b2 in D-layout rows
    __shared__ float2 ldsA2xy[K3 ? kK2Steps * 64 : 1];  // (i, lane) -> W2[{0, 16} + (lane & 15)][4 i + (lane >> 4)]
    __shared__ float ldsA2z[K3 ? kK2Steps * 64 : 1];    // (i, lane) -> W2[32 + (lane & 15)][4 i + (lane >> 4)]
    __shared__ float4 ldsW4849[K3 ? (kK2Steps + 1) * 2 : 1];  // (i + 1, row) -> W2[48 + row][4 i + {0, 1, 2, 3}]; entry (0, row) = 0
    __shared__ float4 ldsB2[3 * 4];                     // (tau, q) -> b2[16 tau + 4 q + {0, 1, 2, 3}]
    __shared__ float ldsB2L[2];                         // b2[48], b2[49]
    __shared__ int4 ldsU[N * NL];  // (phase, slot p) -> the logical states of the lane's four slots at that phase (kept out of the VGPRs)
    // kAlias (S = 4, 8): the k-loop's scratch image lies ON the chunk image (the one is dead while the other is live, provided both
    // tiles' transposes are done before the first logits are written): 34.2 -> 29.9 KB per workgroup at S = 8 = five workgroups
    // per CU instead of four, so that 10 000 blocks (1 250 workgroups) are one round of the chip instead of 1.22 (1.58 -> 1.44 ms);
    // at S = 4 (32.0 -> 26.9 KB) 1.66 -> 1.55 ms.  At 32 / 64 states the 13 more live registers cost more than the LDS buys.
    constexpr bool kAlias = K3 && MVN_IP_ALIAS(LB);
    constexpr int CFA = kAlias && CF < 320 ? 320 : CF;
    __shared__ float4 ldsT[K3 && !kAlias ? kVfWaves : 1][80];  // wave-private: [symbol][k-phase] image of a k-step's sigmoids / transpose image
    __shared__ __attribute__((aligned(16))) float image[kVfWaves][CFA];
    __shared__ unsigned dbits_all[kVfWaves][BPW];  // a chunk's decisions: bit j of word g = step j of block g
    static_assert(CS <= 32, "a chunk's decisions of a block are one word");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: block numbers and image pointers stay scalar
    const int jc = lane & 15, q = lane >> 4;  // the MLP tile's coordinates: symbol column, k / row group
    const int p = lane & (NL - 1), g = lane >> LB;  // the sweep's: slot within the block, block within the wave

    // ---- prologue: W3 / b3 into LDS in A-operand order, W1 / b1 / W2 / b2 into registers (mlp_kernel's layout), and ONE look at
    // every weight: can some but not all branch costs be NaN?
    bool odd = false;
    for (int e = threadIdx.x; e < NT3 * kK3Steps * 64; e += blockDim.x) {
        const int l = e & 63, i3 = (e >> 6) % kK3Steps, j3 = (e >> 6) / kK3Steps;
        const int st = 16 * j3 + (l & 15), k = 4 * i3 + (l >> 4);
        const float w = (st < S && k < kH2) ? W3[st * kH2 + k] : 0.0f;
        ldsA3[e] = w;
        odd |= needs_strict_min(w);
    }
    for (int e = threadIdx.x; e < NT3 * 16; e += blockDim.x) {
        const float w = e < S ? b3[e] : 0.0f;
        ldsB3[e] = w;
        odd |= needs_strict_min(w);
    }
    // W2 as the layer-2 A operands and {-w1, -b1} stay in LDS (vnet16_fusedn.inc: the reads are free next to the MFMAs, the 166
    // registers they took in mlp_kernel are not: 2 waves per SIMD instead of 4)
    for (int e = threadIdx.x; e < kK2Steps * 64; e += blockDim.x) {
        const int l = e & 63, i = e >> 6, k = 4 * i + (l >> 4), u = l & 15;
        const float4 w = make_float4(W2[u * kH1 + k], W2[(16 + u) * kH1 + k], W2[(32 + u) * kH1 + k], 48 + u < kH2 ? W2[(48 + u) * kH1 + k] : 0.0f);
        if constexpr (K3) {
            ldsA2xy[e] = make_float2(w.x, w.y);
            ldsA2z[e] = w.z;
        } else {
            ldsA2[e] = w;
        }
        odd |= needs_strict_min(w.x) | needs_strict_min(w.y) | needs_strict_min(w.z) | needs_strict_min(w.w);
    }
    if constexpr (K3) {
        for (int e = threadIdx.x; e < (kK2Steps + 1) * 2; e += blockDim.x) {
            const float *wr = W2 + (48 + (e & 1)) * kH1 + 4 * ((e >> 1) - (e >= 2 ? 1 : 0));
            ldsW4849[e] = e >= 2 ? make_float4(wr[0], wr[1], wr[2], wr[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (threadIdx.x < 12) {
            const int u0 = 16 * (threadIdx.x >> 2) + 4 * (threadIdx.x & 3);
            ldsB2[threadIdx.x] = make_float4(b2[u0], b2[u0 + 1], b2[u0 + 2], b2[u0 + 3]);
        }
        if (threadIdx.x < 2) ldsB2L[threadIdx.x] = b2[48 + threadIdx.x];
    }
    for (int e = threadIdx.x; e < N * NL; e += blockDim.x) {
        const int rho_ = e >> LB, p_ = e & (NL - 1);
        int u_[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int X = va_ip_coords<LB>(p_, r);
            u_[r] = ((X | (X << N)) >> rho_) & (S - 1);
        }
        ldsU[e] = make_int4(u_[0], u_[1], u_[2], u_[3]);
    }
    float wmax = 0.0f, bmax = 0.0f;
    for (int e = threadIdx.x; e < kK2Steps * 4; e += blockDim.x) {  // (i, q) -> {-w1, -b1}[4 i + q]
        ldsWB[e] = make_float2(-W1[e], -b1[e]);
        odd |= needs_strict_min(W1[e]) | needs_strict_min(b1[e]);
    }
    for (int e = lane; e < kH1; e += 64) {  // every wave for itself: max |w1|, max |b1| (the fast sigmoid's range test)
        wmax = fmaxf(wmax, fabsf(W1[e]));
        bmax = fmaxf(bmax, fabsf(b1[e]));
    }
    float b2v[K3 ? 1 : 4][4];
    if constexpr (K3) {
        if (threadIdx.x < kH2) odd |= needs_strict_min(b2[threadIdx.x]);
    } else {
#pragma unroll
        for (int tau = 0; tau < 4; ++tau)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = 16 * tau + 4 * q + r;
                b2v[tau][r] = u < kH2 ? b2[u] : 0.0f;
                odd |= needs_strict_min(b2v[tau][r]);
            }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        wmax = fmaxf(wmax, __shfl_xor(wmax, off));
        bmax = fmaxf(bmax, __shfl_xor(bmax, off));
    }
    // (also the barrier that publishes the LDS images; the flag goes to a scalar register -- as a vector condition every use of it
    // below became a pair of exec-masked passes)
    const bool strict = __builtin_amdgcn_readfirstlane(__syncthreads_or(odd)) != 0;
    wmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wmax)));  // wave-uniform: scalar registers
    bmax = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(bmax)));

    // wave w of workgroup g takes the w-th row of block groups: the launcher sizes the grid so that a batch that does not fill the
    // chip is spread over all CUs with equally many active waves each (launch_vnet_fused_ip)
    const int64_t b0 = ((int64_t)wave * gridDim.x + blockIdx.x) * BPW;
    if (b0 >= B) return;  // whole wave; nothing below synchronises the workgroup
    const int nvalid = B - b0 < BPW ? (int)(B - b0) : BPW;
    float *img = &image[wave][0];
    unsigned *dbits = &dbits_all[wave][0];

    // image address of (block g, step 0, state 0): see sweep_inplace_kernel.  The lanes of the layout's unused blocks (g >= BPW)
    // shadow block 0: they read valid memory, never write, and no partner operation crosses a block
    auto lane_base_of = [](int lane_) {
        const int g_ = lane_ >> LB, gi = g_ < BPW ? g_ : 0;
        return gi * IMG + 4 * ((gi * IMG) >> 8);
    };

    // ---- the MLP of chunk c's symbols -> the image.  Symbol n = 16 tile + column = g_ * CS + j_ (block-major)
    auto mlp_chunk = [&](int c) {
        if constexpr (!K3) {
        constexpr int TI = vnet_ip_tiles<LB>();  // tiles in flight: their sigmoid chains and MFMAs interleave in one k-loop
        static_assert(NTILE % TI == 0, "whole groups of tiles");
#pragma unroll 1
        for (int tile0 = 0; tile0 < NTILE; tile0 += TI) {
            float yj[TI];
            int fsym[TI];
            bool fast = true;
#pragma unroll
            for (int ti = 0; ti < TI; ++ti) {
                const int n = 16 * (tile0 + ti) + jc, g_ = n / CS, j_ = n % CS;
                int step = CS * c + j_;
                if (step >= T) step = T - 1;                       // partial last chunk: valid data, never used
                const int blk = g_ < nvalid ? g_ : nvalid - 1;     // past the batch: the last block again, never stored
                yj[ti] = y[(b0 + blk) * y_ld + step];
                fsym[ti] = g_ * IMG + j_ * S + 4 * q;  // (block g_, step j_, state 4 q) of the chunk image, before padding
                // the fast sigmoid is exact inside its range (vnet16_common.inc): wave-uniform choice, same bits either way
                fast = fast && __all(fabsf(yj[ti]) * wmax + bmax <= kFastSigmoidBound);
            }
            f32x4 acc[TI][4];
#pragma unroll
            for (int ti = 0; ti < TI; ++ti)
#pragma unroll
                for (int tau = 0; tau < 4; ++tau) acc[ti][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
            auto layer2 = [&](auto sig) {
#pragma unroll
                for (int i = 0; i < kK2Steps; ++i) {
                    const float2 wb = ldsWB[4 * i + q];
                    const float4 a = ldsA2[64 * i + lane];
                    float h[TI];
#pragma unroll
                    for (int ti = 0; ti < TI; ++ti) h[ti] = sig(__builtin_fmaf(yj[ti], wb.x, wb.y));  // -(fma(y,w1,b1)): exp's argument
#pragma unroll
                    for (int ti = 0; ti < TI; ++ti) {
                        acc[ti][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, h[ti], acc[ti][0], 0, 0, 0);
                        acc[ti][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, h[ti], acc[ti][1], 0, 0, 0);
                        acc[ti][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, h[ti], acc[ti][2], 0, 0, 0);
                        acc[ti][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, h[ti], acc[ti][3], 0, 0, 0);
                    }
                }
            };
            if (fast) layer2([](float d) { return sigmoid_from_neg_fast(d); });
            else layer2([](float d) { return sigmoid_from_neg(d); });
#pragma unroll
            for (int ti = 0; ti < TI; ++ti) {
                // bias + ReLU in the D layout, then the (q, r) transpose into B-operand order (mlp_kernel)
                float bop[16];
#pragma unroll
                for (int tau = 0; tau < 4; ++tau) {
                    unsigned u[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float z = acc[ti][tau][r] + b2v[tau][r];
                        u[r] = __float_as_uint(z < 0.0f ? 0.0f : z);  // relu; NaN propagates like torch's
                    }
                    u32x2 pp;
                    pp = __builtin_amdgcn_permlane32_swap(u[0], u[2], false, false);
                    u[0] = pp[0];
                    u[2] = pp[1];
                    pp = __builtin_amdgcn_permlane32_swap(u[1], u[3], false, false);
                    u[1] = pp[0];
                    u[3] = pp[1];
                    pp = __builtin_amdgcn_permlane16_swap(u[0], u[1], false, false);
                    u[0] = pp[0];
                    u[1] = pp[1];
                    pp = __builtin_amdgcn_permlane16_swap(u[2], u[3], false, false);
                    u[2] = pp[0];
                    u[3] = pp[1];
#pragma unroll
                    for (int r = 0; r < 4; ++r) bop[4 * tau + r] = __uint_as_float(u[r]);
                }
#pragma unroll 1
                for (int j3 = 0; j3 < NT3; ++j3) {
                    f32x4 acc3 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i3 = 0; i3 < kK3Steps; ++i3)
                        acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(ldsA3[(j3 * kK3Steps + i3) * 64 + lane], bop[i3], acc3, 0, 0, 0);
                    const int st0 = 16 * j3 + 4 * q;
                    if (st0 < S) {  // (S = 4, 8: the tile's upper states do not exist)
                        const int f = fsym[ti] + 16 * j3;
                        float4 v;
                        v.x = acc3[0] + ldsB3[st0 + 0];
                        v.y = acc3[1] + ldsB3[st0 + 1];
                        v.z = acc3[2] + ldsB3[st0 + 2];
                        v.w = acc3[3] + ldsB3[st0 + 3];
                        *reinterpret_cast<float4 *>(&img[f + 4 * (f >> 8)]) = v;
                    }
                }
            }
        }
        }
    };
#ifdef MVN_DIAG_PHASES  // diagnostic build only (tools/diag_phases_ip.py): cycles per phase, summed over the wave's chunks
    unsigned long long dg[4] = {0, 0, 0, 0}, dg_t = __builtin_amdgcn_s_memtime();
#define MVN_IP_STAMP(K)                                                  \
    {                                                                    \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();    \
        dg[K] += now_ - dg_t;                                            \
        dg_t = now_;                                                     \
    }
#else
#define MVN_IP_STAMP(K)
#endif
    // ---- the same at S <= 64 with vnet16_fusedn.inc's k-loop (NT = 2: the chunk's two tiles in flight; see there for the chain
    // image's protocol).  Symbols and image layout as in mlp_chunk; the next chunk's inputs are requested one chunk ahead.
    float ynext[2] = {0.0f, 0.0f};
    auto fetch_y = [&](int c) {
        if constexpr (K3) {
            int lane_y = lane;  // (opaque: the row addresses are formed here, once per chunk, not held across the loop)
            asm volatile("" : "+v"(lane_y));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int n = 16 * u + (lane_y & 15);
                const int g_ = HALF ? (lane_y & 15) / HS : n / CS, j_ = HALF ? HS * u + (lane_y & 15) % HS : n % CS;
                int step = CS * c + j_;
                if (step >= T) step = T - 1;                    // partial last chunk / past the end: valid data, never used
                const int blk = g_ < nvalid ? g_ : nvalid - 1;  // past the batch: the last block again, never stored
                ynext[u] = y[(b0 + blk) * y_ld + step];
            }
        }
    };
    f32x4 acc[2][3];     // the chunk's two tiles: hidden-2 units 0..47 in the MFMA's D layout
    float hl[2];         // ... units 48 / 49 in layer 3's operand layout
    float bops[2][13];   // a tile's layer-3 B operands
    auto kloop = [&](int c) {
        static_assert(!K3 || (vnet_ip_tiles<LB>() == 2 && NTILE == 2), "the two tiles of a chunk are the k-loop's two tiles in flight");
        // per-lane LDS addresses from an opaque copy of the lane id, once per chunk: nothing of them stays in registers across the sweep
        int lane_k = lane;
        asm volatile("" : "+v"(lane_k));
        const int qk = lane_k >> 4;
        float4 *const tbase = kAlias ? reinterpret_cast<float4 *>(img) : &ldsT[K3 && !kAlias ? wave : 0][0];
        float *const tbw = reinterpret_cast<float *>(tbase) + 4 * (lane_k & 15) + qk;  // + 64 u: (symbol 16 u + j, k-phase q)
        float4 *const tbr = tbase + (lane_k & 31);                                      // this lane's chain symbol
        const float4 *const wch = &ldsW4849[K3 ? (lane_k >> 5) : 0];                    // + 2 (i + 1): unit 48 (lanes 0..31) / 49
        float yv[2] = {ynext[0], ynext[1]};
        fetch_y(c + 1);
        const bool fast = __all(fmaxf(fabsf(yv[0]), fabsf(yv[1])) * wmax + bmax <= kFastSigmoidBound);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int tau = 0; tau < 3; ++tau) acc[u][tau] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ca = 0.0f;  // this lane's unit chain
        *tbr = make_float4(0.f, 0.f, 0.f, 0.f);  // "k-step -1" of the chain image (it held the previous chunk's transposes)
        wave_lds_fence();
        auto chain_step = [&](const float4 tr, const float4 wa) {
            ca = __builtin_fmaf(wa.x, tr.x, ca);
            ca = __builtin_fmaf(wa.y, tr.y, ca);
            ca = __builtin_fmaf(wa.z, tr.z, ca);
            ca = __builtin_fmaf(wa.w, tr.w, ca);
        };
        auto layer2 = [&](auto sigmoid) {
            for (int i0 = 0; i0 < kK2Steps; i0 += 5) {
#pragma unroll
                for (int ii = 0; ii < 5; ++ii) {
                    const int i = i0 + ii;
                    const float2 axy = ldsA2xy[i * 64 + lane_k];
                    const float az = ldsA2z[i * 64 + lane_k];
                    const float2 wb = ldsWB[i * 4 + qk];
                    // the image still holds k-step i - 1: request it now, consume it after this k-step's sigmoids.  (k-step 0 finds
                    // zeros in the image and in the weights' entry 0: fmaf(0, 0, 0) four times -- no first trip of its own, which
                    // the compiler would peel off the loop at the price of a dozen registers)
                    const float4 tr = *tbr, wa = wch[2 * i];
                    wave_lds_fence();
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const float h = sigmoid(__builtin_fmaf(yv[u], wb.x, wb.y));
                        acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(axy.x, h, acc[u][0], 0, 0, 0);
                        acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(axy.y, h, acc[u][1], 0, 0, 0);
                        acc[u][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(az, h, acc[u][2], 0, 0, 0);
                        tbw[64 * u] = h;
                        __builtin_amdgcn_sched_barrier(0);  // keep the sigmoids from interleaving (registers)
                    }
                    chain_step(tr, wa);
                    wave_lds_fence();
                }
            }
            wave_lds_fence();
            chain_step(*tbr, wch[2 * kK2Steps]);
        };
        if (fast) layer2([](float d) { return sigmoid_from_neg_fast(d); });
        else layer2([](float d) { return sigmoid_from_neg(d); });

        // units 48, 49 -> bias + ReLU -> back through the image: tile u's layer-3 operand wants h2[48 + q] of symbol 16 u + j at row q
        {
            wave_lds_fence();
            const float za = ca + ldsB2L[lane_k >> 5];
            float *slot = reinterpret_cast<float *>(tbr) + (lane_k >> 5);
            slot[0] = za < 0.0f ? 0.0f : za;
            slot[2] = 0.0f;
            wave_lds_fence();
            hl[0] = tbw[0];
            hl[1] = tbw[64];
            wave_lds_fence();
        }
#if MVN_IP_PRIO
        __builtin_amdgcn_s_setprio(3);  // layer 3 and the sweep: short dependent bursts between LDS round trips
#endif
        MVN_IP_STAMP(0);
    };
    auto transpose_tile = [&](auto u_c) {  // acc[u], hl[u] -> bops[u]
        constexpr int u = decltype(u_c)::value;
        {
            int lane_t = lane;
            asm volatile("" : "+v"(lane_t));
            const int jt = lane_t & 15, qt = lane_t >> 4;
            float4 *const tbase = kAlias ? reinterpret_cast<float4 *>(img) : &ldsT[K3 && !kAlias ? wave : 0][0];
            float4 *const ttw = tbase + 5 * jt + qt;                                        // transpose image: row j, units 4 q .. 4 q + 3
            const float *const ttr = reinterpret_cast<const float *>(tbase + 5 * jt) + qt;  // + 4 r': unit 4 r' + q of row j
            float (&bop)[13] = bops[u];
            // bias + ReLU in the D layout (lane (j, q), register r = unit 16 tau + 4 q + r of symbol j), then the (q, r) transpose
            // into layer 3's operand order through the wave's image (LDS instructions cost the FP32 pipe nothing)
#pragma unroll
            for (int tau = 0; tau < 3; ++tau) {
                const float4 bb = ldsB2[tau * 4 + qt];
                const float bbr[4] = {bb.x, bb.y, bb.z, bb.w};
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = acc[u][tau][r] + bbr[r];
                    v[r] = z < 0.0f ? 0.0f : z;  // relu; NaN propagates like torch's
                }
                *ttw = make_float4(v[0], v[1], v[2], v[3]);
                wave_lds_fence();
#pragma unroll
                for (int r = 0; r < 4; ++r) bop[4 * tau + r] = ttr[4 * r];
                wave_lds_fence();
            }
            bop[12] = hl[u];
        }
    };
    auto layer3_tile = [&](auto u_c) {  // bops[u] -> the tile's logits in the chunk image
        constexpr int u = decltype(u_c)::value;
        {
            int lane_t = lane;
            asm volatile("" : "+v"(lane_t));
            const int jt = lane_t & 15, qt = lane_t >> 4;
            const float (&bop)[13] = bops[u];
            const int n = 16 * u + jt;  // (block, step, state 4 q) of the chunk image:
            const int fs = (HALF ? jt / HS : n / CS) * IMG + (HALF ? jt % HS : n % CS) * S + 4 * qt;
#pragma unroll 1
            for (int j3 = 0; j3 < NT3; ++j3) {
                f32x4 acc3 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i3 = 0; i3 < kK3Steps; ++i3)
                    acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(ldsA3[(j3 * kK3Steps + i3) * 64 + lane_t], bop[i3], acc3, 0, 0, 0);
                const int st0 = 16 * j3 + 4 * qt;
                if (st0 < S) {  // (S = 4, 8: the tile's upper states do not exist)
                    const int f = fs + 16 * j3;
                    float4 v;
                    v.x = acc3[0] + ldsB3[st0 + 0];
                    v.y = acc3[1] + ldsB3[st0 + 1];
                    v.z = acc3[2] + ldsB3[st0 + 2];
                    v.w = acc3[3] + ldsB3[st0 + 3];
                    *reinterpret_cast<float4 *>(&img[f + 4 * (f >> 8)]) = v;
                }
            }
        }
    };
    auto flush = [&](int c) {  // decisions of chunk c: rows of CS steps, float4 per lane when the rows are 16-byte aligned
        const int t0 = CS * c;
        int lane_f = lane;
        asm volatile("" : "+v"(lane_f));
#pragma unroll
        for (int it = 0; it < NS; ++it) {
            const int k = it * 64 + lane_f, blk = k / (CS / 4), q4 = k % (CS / 4);
            if (BPW * (CS / 4) > k && blk < nvalid) {
                const unsigned bits = dbits[blk] >> (4 * q4);
                float *dp = dec + (b0 + blk) * dec_ld + t0 + 4 * q4;
                if (aligned && t0 + 4 * q4 + 3 < T) {
                    *reinterpret_cast<float4 *>(dp) = make_float4((float)(bits & 1u), (float)((bits >> 1) & 1u),
                                                                  (float)((bits >> 2) & 1u), (float)((bits >> 3) & 1u));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (t0 + 4 * q4 + e < T) dp[e] = (float)((bits >> e) & 1u);
                }
            }
        }
    };

    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // vnet_detector.py:51
    const float *img_lane = img;  // + the lane's block: set per chunk from an opaque lane id (not held across the k-loop)
    unsigned dbit = 0;            // the chunk's decisions so far (every lane of a block computes the same bits)
    // trellis step j (an int, or an integral_constant) of the current chunk at phase RHO; maybe_strict = false_type: the plain minimum
    auto stage = [&](auto rho_c, auto j_, auto maybe_strict) {
        constexpr int RHO = decltype(rho_c)::value;
        const int j = j_;
        const bool strict_ = decltype(maybe_strict)::value && strict;
        const int jj = HALF ? (j & (HS - 1)) : j;  // the step's row of the chunk image
        const float *row = img_lane + jj * S + 4 * ((jj * S) >> 8);
        const int4 u4 = ldsU[RHO * NL + (lane & (NL - 1))];
        const int u[4] = {u4.x, u4.y, u4.z, u4.w};
        float a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = m[r] - row[u[r]];  // branch cost = -logit (vnet_detector.py:57)
        // decision from the metrics BEFORE this stage (vnet_detector.py:55)
        const int bit = strict_ ? va_ip_decide_strict_u<LB, RHO>(m, u, lane) : va_ip_decide_u<LB, RHO>(m, u, lane);
        dbit |= (unsigned)bit << j;
        if (strict_) va_ip_acs_strict<LB, RHO>(m, a, lane);
        else va_ip_acs<LB, RHO>(m, a, lane);
    };

    const int nchunks = (T + CS - 1) / CS;
    int rho = 0;
    fetch_y(0);
#if MVN_IP_PRIO
    const int third = (nchunks + 2) / 3;
#endif
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;
#pragma unroll 1
    for (int c = 0; c < nchunks; ++c) {
        if constexpr (K3) {
#if MVN_IP_PRIO  // (vnet16_fusedn.inc's two rules: the k-loop's priority falls with the wave's progress, the rest runs at the top)
            if (c < third) __builtin_amdgcn_s_setprio(2);
            else if (c < 2 * third) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
#endif
            kloop(c);
            if constexpr (kAlias || HALF) {  // the scratch image lies on the chunk image: both tiles leave it before logits arrive
                transpose_tile(T0{});
                transpose_tile(T1{});
            }
        }
        dbit = 0;
#pragma unroll
        for (int h = 0; h < CS / HS; ++h) {  // the chunk image's fills: one, or one per tile (HALF)
            if constexpr (!K3) {
                mlp_chunk(c);
            } else if constexpr (HALF) {
                if (h == 0) layer3_tile(T0{});
                else layer3_tile(T1{});
            } else if constexpr (kAlias) {
                layer3_tile(T0{});
                layer3_tile(T1{});
            } else {
                transpose_tile(T0{});
                layer3_tile(T0{});
                transpose_tile(T1{});
                layer3_tile(T1{});
            }
            wave_lds_fence();
            MVN_IP_STAMP(1);
            {
                int lane_s = lane;
                asm volatile("" : "+v"(lane_s));
                img_lane = img + lane_base_of(lane_s);
            }
            // A whole chunk with the plain minimum (all of them but a word's last, in practice): its CS steps unrolled, one copy per
            // starting phase -- phases, image rows and decision bits are then immediates: ~15-30 instructions per step without a
            // branch, where the loop below spends ~75 with eight taken branches (the sweep was a third of the kernel's time).
            constexpr bool kUnrolledSweep = K3 && !HALF && LB <= 4 && MVN_IP_UNROLL;
            if (kUnrolledSweep && !strict && CS * (c + 1) <= T) {
                auto whole_chunk = [&](auto rho0_c) {
                    static_for_each([&](auto j_c) {
                        constexpr int J = decltype(j_c)::value;
                        stage(std::integral_constant<int, (decltype(rho0_c)::value + J) % N>{}, std::integral_constant<int, J>{}, std::false_type{});
                    }, std::make_integer_sequence<int, CS>{});
                };
                switch (rho) {
                    case 0: whole_chunk(std::integral_constant<int, 0>{}); break;
                    case 1: whole_chunk(std::integral_constant<int, 1>{}); break;
                    case 2: if constexpr (N > 2) whole_chunk(std::integral_constant<int, 2>{}); break;
                    case 3: if constexpr (N > 3) whole_chunk(std::integral_constant<int, 3>{}); break;
                    case 4: if constexpr (N > 4) whole_chunk(std::integral_constant<int, 4>{}); break;
                    default: if constexpr (N > 5) whole_chunk(std::integral_constant<int, 5>{}); break;
                }
                rho = (rho + CS) % N;
            } else
#pragma unroll 1
            for (int j = h * HS; j < (h + 1) * HS; ++j) {
                if (CS * c + j >= T) break;  // wave-uniform
                switch (rho) {
                    case 0: stage(std::integral_constant<int, 0>{}, j, std::true_type{}); break;
                    case 1: stage(std::integral_constant<int, 1>{}, j, std::true_type{}); break;
                    case 2: if constexpr (N > 2) stage(std::integral_constant<int, 2>{}, j, std::true_type{}); break;
                    case 3: if constexpr (N > 3) stage(std::integral_constant<int, 3>{}, j, std::true_type{}); break;
                    case 4: if constexpr (N > 4) stage(std::integral_constant<int, 4>{}, j, std::true_type{}); break;
                    case 5: if constexpr (N > 5) stage(std::integral_constant<int, 5>{}, j, std::true_type{}); break;
                    case 6: if constexpr (N > 6) stage(std::integral_constant<int, 6>{}, j, std::true_type{}); break;
                    default: if constexpr (N > 7) stage(std::integral_constant<int, 7>{}, j, std::true_type{}); break;
                }
                rho = rho + 1 == N ? 0 : rho + 1;
            }
            if constexpr (HALF) wave_lds_fence();  // the half's image reads have landed before the next tile's logits overwrite it
        }
        if ((lane & (NL - 1)) == 0 && (lane >> LB) < BPW) dbits[lane >> LB] = dbit;
        wave_lds_fence();  // every read of the image has landed, the decisions are in dbits
        MVN_IP_STAMP(2);
        flush(c);
        wave_lds_fence();  // (dbits is rewritten by the next chunk)
        MVN_IP_STAMP(3);
    }
#ifdef MVN_DIAG_PHASES
    if (final_metric && lane == 0 && nvalid == BPW) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(final_metric + b0 * S);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = dg[k];
    }
    return;
#endif
    if (g < nvalid && final_metric) {
        const int rf = T % N;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int X = va_ip_coords<LB>(p, r);
            final_metric[(b0 + g) * S + (((X | (X << N)) >> rf) & (S - 1))] = m[r];
        }
    }
}

// -1 = not served (S = 2 or 16): the caller takes its other routes
inline bool vnet_fused_ip_serves(int S) { return S == 4 || S == 8 || S == 32 || S == 64 || S == 128 || S == 256; }
inline int launch_vnet_fused_ip(const float *y, int64_t y_ld, const float *W1, const float *b1, const float *W2, const float *b2,
                                const float *W3, const float *b3, float *dec, int64_t dec_ld, float *final_metric, int64_t B, int T,
                                int S, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
    const int aligned = !((reinterpret_cast<uintptr_t>(dec) & 15) || (dec_ld & 3));  // float4 decision stores, else one by one
    const int64_t cus = current_device_cus();
#define MVN_VF_CASE(LB)                                                                                                    \
    {                                                                                                                      \
        const int64_t W = vnet_ip_waves<LB>(), groups = (B + vnet_ip_blocks<LB>() - 1) / vnet_ip_blocks<LB>();           \
        const int64_t dense = (groups + W - 1) / W, per_cu = (groups + W * cus - 1) / (W * cus);                            \
        /* one round of the chip or less: k workgroups on every CU, their waves equally loaded; more: full workgroups */    \
        const int64_t grid = per_cu <= vnet_ip_wgs<LB>() ? (groups < cus * per_cu ? groups : cus * per_cu) : dense;          \
        hipLaunchKernelGGL((vnet_fused_ip_kernel<LB>), dim3((unsigned)grid), dim3(64 * vnet_ip_waves<LB>()), 0, st, y,     \
                           y_ld, W1, b1, W2, b2, W3, b3, dec, dec_ld, final_metric, B, T, aligned);                        \
        return (int)hipGetLastError();                                                                                     \
    }
    switch (S) {
        case 4: MVN_VF_CASE(0)
        case 8: MVN_VF_CASE(1)
        case 32: MVN_VF_CASE(3)
        case 64: MVN_VF_CASE(4)
        case 128: MVN_VF_CASE(5)
        case 256: MVN_VF_CASE(6)
        default: return -1;
    }
#undef MVN_VF_CASE
}
