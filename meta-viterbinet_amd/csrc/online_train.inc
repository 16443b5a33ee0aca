// online_train.inc -- persistent on-chip training of the ViterbiNet MLP (SURVEY 8f next #3), included by
// mvn_hip.hip inside its anonymous namespace.
//
// Counterpart of the self-supervised / online training loop the by-word evaluation runs after every block:
//   VNETTrainer.online_training (python_code/trainers/VNET/vnet_trainer.py:49-60) -> Trainer.run_train_loop
//   (trainers/trainer.py:492-505): n_iter x { logits = net(rx) ; CE(logits[idx], states[idx]) ; backward ;
//   Adam.step }, with idx a 32-sample minibatch (select_batch, trainer.py:534-544), or all T samples
//   (metavnet_trainer.py:41-64).
// The reference issues ~40 tiny ATen kernels per iteration; here ONE workgroup keeps the 6 066 parameters,
// both Adam moments and all activations in LDS (<= 160 KB) and runs all iterations in a single launch.
// The matrix products of the forward and backward pass (three of 160 k multiply-adds per 32-sample chunk, and
// four smaller ones) run as 16x16 tiles of v_mfma_f32_16x16x4_f32 with operands read straight from LDS, one
// tile per wave; the elementwise parts, the loss and Adam stay on the vector ALU.
// fp32 throughout; reductions run in a fixed order (deterministic), but not torch's order, so results agree
// with torch autograd + torch.optim.Adam to rounding (tolerance stated in the tests), not bit for bit.
constexpr int kTrainThreads = 1024;
constexpr int kTrainChunk = 32;  // samples processed per pass (select_batch's minibatch size)

// Row strides of the activation images.  z2 / dz2 rows carry two zero columns (the 50-long contraction runs in 13
// k-steps of 4) and a dlogits row is 34 wide with zeros beyond S (the contraction over states runs in 4 or 8 k-steps):
// padded operands are exact zeros, so whatever finite value the other operand picks up there contributes nothing.
// All row strides are 2 x odd: the 16 rows a product's lanes read side by side (stride x row + k, k = l >> 4 in {0,1} or {2,3}
// within a 32-lane half) then fall on 32 different banks of ds_read_b32's 32 (round 2 used 100 / 52 / 33-float rows: rows r and
// r + 8 shared their banks, every operand read of the forward products took two LDS passes = ~50 cycles per MFMA).
constexpr int kH1Ld = kH1 + 2;      // h1 / dz1 images and W2's rows in the LDS parameter vectors
constexpr int kZ2Stride = kH2 + 4;  // 54
constexpr int kDlStride = 34;
// Up to this many states W3's gradient lies in the LDS gradient vector g[]; above (256) it stays in registers (grad_chunk, SCC = 256)
// and g[] ends with db3 where dW3 would begin.
constexpr int kGradW3InLdsStates = 128;

struct TrainLayout {  // offsets (floats) of the six parameter arrays inside one LDS vector [P], torch order, W2's rows padded
    int w1, b1, w2, b2, w3, b3, P, P4, Pflat;  // Pflat: length of the unpadded vector (the Adam moments in global memory)
};
// LDS index of element e of the flat torch-order vector (W1 [100], b1 [100], W2 [50][100], b2 [50], W3 [S][50], b3 [S])
__host__ __device__ inline int lds_index(int e) {
    constexpr int w2_flat = 2 * kH1, w2_end = w2_flat + kH2 * kH1;
    if (e < w2_flat) return e;
    if (e < w2_end) return w2_flat + ((e - w2_flat) / kH1) * kH1Ld + (e - w2_flat) % kH1;
    return e + kH2 * (kH1Ld - kH1);
}
__host__ __device__ inline TrainLayout train_layout(int S) {
    TrainLayout L;
    L.w1 = 0;
    L.b1 = L.w1 + kH1;
    L.w2 = L.b1 + kH1;
    L.b2 = L.w2 + kH2 * kH1Ld;  // W2's rows are kH1Ld apart in LDS (bank-conflict-free operand reads), 100 apart in global memory
    L.w3 = L.b2 + kH2;
    L.b3 = L.w3 + S * kH2;
    L.P = L.b3 + S;
    L.P4 = (L.P + 3) & ~3;  // the four flat arrays are padded to whole float4s (Adam runs on 16-byte LDS accesses)
    L.Pflat = L.P - kH2 * (kH1Ld - kH1);
    return L;
}
#ifdef MVN_ABLATE  // diagnostic builds only (tools/ablate_train.py): phase K's body compiled out, its barrier kept (wrong results)
#define MVN_ABL(K) ((MVN_ABLATE) == (K))
#else
#define MVN_ABL(K) false
#endif
#ifdef MVN_DIAG_TRAIN  // diagnostic build only (tools/prof_train_phases.py): s_memtime at the phase boundaries of iteration 100
__device__ unsigned long long g_diag_stamps[24 + 8 * 16];
__device__ int g_diag_on;
#define TRAIN_STAMP(K)                                                                  \
    do {                                                                                \
        if (threadIdx.x == 0 && g_diag_on) g_diag_stamps[K] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// every wave's own stamp (slot 24 + 16 PH + wave): when it reached the barrier that ends phase PH (0 .. 7)
#define TRAIN_STAMP_WAVE(PH)                                                                                                \
    do {                                                                                                                    \
        if ((threadIdx.x & 63) == 0 && g_diag_on) g_diag_stamps[24 + 16 * (PH) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define TRAIN_STAMP(K) do {} while (0)
#define TRAIN_STAMP_WAVE(PH) do {} while (0)
#endif

// N sigmoids of a thread.  The fast form (vnet16_common.inc) is exact inside its range |z| <= 86 -- the same value as the full
// form, bit for bit -- so which of the two runs cannot be seen in the result: the wave takes the fast form when ALL its lanes are
// inside the range (always, in practice) and the full form for all lanes otherwise.  (Round 3 selected per lane, which makes the
// compiler evaluate BOTH forms for every element: 55 instead of 20 instructions per sigmoid, a third of a chunk's vector work.)
template <int N>
__device__ __forceinline__ void sigmoid_train_n(const float (&z)[N], float (&h)[N]) {
    bool wide = false;
#pragma unroll
    for (int j = 0; j < N; ++j) wide |= !(fabsf(z[j]) <= kFastSigmoidBound);  // (a NaN is "wide": the full form propagates it)
    if (__any(wide)) {
#pragma unroll
        for (int j = 0; j < N; ++j) h[j] = sigmoid_from_neg(0.0f - z[j]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) h[j] = sigmoid_from_neg_fast(0.0f - z[j]);
    }
}
__device__ __forceinline__ float sigmoid_train(float z) {
    const float zz[1] = {z};
    float h[1];
    sigmoid_train_n<1>(zz, h);
    return h[0];
}

// One 16x16 output tile D = A . B on v_mfma_f32_16x16x4_f32 with both operands in LDS, contraction length 4 KS.
// Lane l supplies A(i, k) and B(k, j) for i = j = l & 15, k = 4 ks + (l >> 4) and receives D[4 (l >> 4) + r][l & 15]
// in acc[r].  a_lane / b_lane point at the lane's k = (l >> 4) element; SA_K / SB_K are the k strides (floats), so
// every further operand is an immediate offset away.  Operands of up to 8 k-steps are fetched together (one LDS
// round trip), then their MFMAs run.
// ROWS_K = true: the contraction runs over the ROWS of both images (gradient products: SA_K / SB_K are row strides and each
// lane reads 16 consecutive columns).  The two lane groups of a 32-lane half must then sit 16 banks apart = 8 rows for the
// 2 x odd strides above: k-step ks takes row rows_k_base(l >> 4) + ks (a_lane / b_lane point at row rows_k_base).
template <int KS>
__device__ __forceinline__ int rows_k_base(int lq) {
    static_assert(KS == 8 || KS == 4, "32- or 16-row chunks");
    return KS == 8 ? 8 * lq : 8 * (lq & 1) + 4 * (lq >> 1);
}
template <int KS, int SA_K, int SB_K, bool RELU_A, bool RELU_B, bool ROWS_K = false>
__device__ __forceinline__ f32x4 lds_tile_mfma(const float *a_lane, const float *b_lane) {
    auto koff = [](int ks) { return ROWS_K ? ks : 4 * ks; };
    // two accumulators (even / odd k-steps; the summation order the golden tolerances were taken with -- a dependent chain
    // of f32 MFMAs issues at the full rate of one per 32 cycles, tools/ubench3.hip "chain")
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int G = 8;
#pragma unroll
    for (int k0 = 0; k0 < KS; k0 += G) {
        float a[G], b[G];
#pragma unroll
        for (int ks = 0; ks < G; ++ks) {
            a[ks] = k0 + ks < KS ? a_lane[koff(k0 + ks) * SA_K] : 0.0f;
            b[ks] = k0 + ks < KS ? b_lane[koff(k0 + ks) * SB_K] : 0.0f;
        }
        // all 16 operands live here: keeps the compiler from sinking the reads next to their MFMA (it otherwise
        // waits for LDS once per two k-steps).  Issuing all 2 KS reads of a tile up front instead was measured: no gain --
        // the tile products run at ~50 cycles per MFMA because the LDS delivers their 512 B of operands no faster.
        asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                          "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
#pragma unroll
        for (int ks = 0; ks < G; ++ks)
            if (k0 + ks < KS) {
                const float av = RELU_A ? fmaxf(a[ks], 0.0f) : a[ks], bv = RELU_B ? fmaxf(b[ks], 0.0f) : b[ks];
                if (ks & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc1, 0, 0, 0);
                else acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += acc1[r];
    return acc;
}

// NA x NB adjacent output tiles by ONE wave: the operands of a k-step group are fetched once and every A operand meets every B
// operand, so the LDS bytes per MFMA drop to (NA + NB) / (2 NA NB) of lds_tile_mfma's (1/2 for 2 x 2, 3/4 for 2 x 1).  Every tile
// accumulates exactly as lds_tile_mfma does (even k-steps in one accumulator, odd ones in another, added at the end): the same
// bits, whoever computes it.
template <int KS, int SA_K, int SB_K, bool RELU_A, bool RELU_B, bool ROWS_K, int NA, int NB>
__device__ __forceinline__ void lds_block_mfma(const float *const (&a_lane)[NA], const float *const (&b_lane)[NB],
                                               f32x4 (&out)[NA][NB]) {
    auto koff = [](int ks) { return ROWS_K ? ks : 4 * ks; };
    f32x4 acc[NA][NB], acc1[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float a[NA][KS], b[NB][KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int i = 0; i < NA; ++i) a[i][ks] = a_lane[i][koff(ks) * SA_K];
#pragma unroll
        for (int j = 0; j < NB; ++j) b[j][ks] = b_lane[j][koff(ks) * SB_K];
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float av = RELU_A ? fmaxf(a[i][ks], 0.0f) : a[i][ks];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float bv = RELU_B ? fmaxf(b[j][ks], 0.0f) : b[j][ks];
                if (ks & 1) acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc1[i][j], 0, 0, 0);
                else acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[i][j], 0, 0, 0);
            }
        }
    }
    // the schedule: the operand reads of kPre k-steps, then one k-step of MFMAs per further k-step of reads
    constexpr int kPre = 3;
    __builtin_amdgcn_sched_group_barrier(0x100, kPre * (NA + NB), 0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        __builtin_amdgcn_sched_group_barrier(0x008, NA * NB, 0);
        if (ks + kPre < KS) __builtin_amdgcn_sched_group_barrier(0x100, NA + NB, 0);
    }
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] += acc1[i][j][r];
            out[i][j] = acc[i][j];
        }
}

// LDS images of one chunk of ROWS samples (ROWS = 32 or 16): inputs, activations and their gradients.
template <int ROWS>
struct ChunkArena {
    float *ys;   // [ROWS] chunk inputs
    float *h1;   // [ROWS][100]
    float *z2;   // [ROWS][52] pre-activation, columns 50,51 = 0
    float *dl;   // [ROWS][33] logits -> dlogits, columns >= S = 0
    float *dz2;  // [ROWS][52], columns 50,51 = 0
    float *part;  // [2][ROWS / 16][128]: per row tile, column sums of dz1 (-> db1) and of dz1 * y (-> dW1)
    float *red;  // [ROWS] per-sample loss, [ROWS] running loss, [ROWS + 1] step size, [ROWS + 2] 1/sqrt(bias correction 2)
    int *lab;    // [ROWS] chunk labels
    static constexpr int kPartFloats = 2 * (ROWS / 16) * 128;
    // dls: floats per dlogits row -- kDlStride up to 32 states, n_states + 2 above (grad_chunk's SCC)
    static constexpr int floats(int dls) { return ROWS + ROWS * (kH1Ld + 2 * kZ2Stride + dls) + kPartFloats + ROWS + 3 + ROWS; }
    static constexpr int kFloats = floats(kDlStride);
    // compact: `part` lies on `dl` -- the column sums are written in the hidden-layer backward phase, when the dlogits have been
    // consumed, and read in the closing step, long before the next chunk's logits are written (the form two workgroups per CU
    // need).  16 states only: there every dlogits column a product reads (0..15) is rewritten by the next chunk; with fewer states
    // the columns up to 15 are zero padding that this would destroy.
    static constexpr int kFloatsCompact = kFloats - kPartFloats;
    static_assert(ROWS * kDlStride >= kPartFloats, "part must fit the dlogits image");
    __device__ explicit ChunkArena(float *base, bool compact = false, int dls = kDlStride) {
        ys = base;
        h1 = ys + ROWS;
        z2 = h1 + ROWS * kH1Ld;
        dl = z2 + ROWS * kZ2Stride;
        dz2 = dl + ROWS * dls;
        part = compact ? dl : dz2 + ROWS * kZ2Stride;
        red = dz2 + ROWS * kZ2Stride + (compact ? 0 : kPartFloats);
        lab = (int *)(red + ROWS + 3);
    }
};

// max / sum over the S consecutive lanes of a sample (S a power of two <= 32), result in every lane.  The xor butterfly of
// __shfl_xor (same pairings, so the same sums bit for bit), with the steps inside a 16-lane row as DPP operands instead
// of ds_bpermute round trips (8 of them were 1 000 cycles of the loss phase).
template <bool MAX>
__device__ __forceinline__ float sample_allreduce(float v, int S) {
    auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
    if (S > 1) v = op(v, dpp_f32<MVN_DPP_XOR1>(v));
    if (S > 2) v = op(v, dpp_f32<MVN_DPP_XOR2>(v));
    if (S > 4) v = op(v, dpp_f32<MVN_DPP_XOR7>(v));  // the other quad of the half row: all its lanes hold the same value
    if (S > 8) v = op(v, dpp_f32<MVN_DPP_XOR8>(v));
    if (S > 16) v = op(v, __shfl_xor(v, 16));
    return v;
}

// sum over the wave's four 16-lane rows (lanes l, l + 16, l + 32, l + 48), result in every lane: two v_permlane*_swap
// (odd rows <-> even rows, upper half <-> lower half) instead of LDS round trips
__device__ __forceinline__ float sum_over_rows(float x) {
    const unsigned xu = __float_as_uint(x);
    const auto s16 = __builtin_amdgcn_permlane16_swap(xu, xu, false, false);  // [x0 x0 x2 x2], [x1 x1 x3 x3]
    const float t = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
    const unsigned tu = __float_as_uint(t);
    const auto s32 = __builtin_amdgcn_permlane32_swap(tu, tu, false, false);  // [t0 t1 t0 t1], [t2 t3 t2 t3]
    return __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
}

// Forward + backward of one chunk whose inputs (A.ys, A.lab) are in place: adds the chunk's share of the gradient of the
// mean CrossEntropyLoss over n samples (inv_n = 1/n) to g[] -- `first` (uniform): WRITES it, g[] need not be zero beforehand
// (its padding entries are never touched) -- and its summed loss to A.red[ROWS].  Rows >= nc are padding:
// they run through the network but their dlogits are zeroed, so they add nothing.  p / g: parameter and gradient
// vectors in LDS (TrainLayout).  All kTrainThreads threads call it; it ends with a barrier, before which every thread runs
// closing_hook(): A.ys and A.lab are no longer read by then, so the caller can stage the next chunk's samples there instead of
// in a step (and behind a barrier) of its own.  idle_hook() is run by the last
// lane of the last wave while that wave has nothing to do (first matrix product): a slot for scalar side work.
struct NoHook {
    __device__ void operator()() const {}
};
// ROWS = 32: a full chunk.  ROWS = 16: a chunk whose samples all sit in rows 0..15 (nc <= 16: the tail of a word whose length
// is not a multiple of 32 -- 8 of 136 symbols at the reference's defaults): the same images (the arena keeps its 32-row layout,
// rows 16..31 are neither written nor read), one row tile instead of two in every product, half the k-steps in the products
// that contract over the samples -- 55-60 % of a full chunk's time instead of 100 % for a quarter of its samples.
// FIRST is a compile-time constant on purpose: with a run-time flag every epilogue carries the LDS read of g[] it may not need
// (one more round trip in the critical path of every phase: +9 % per chunk, measured).
// NT: threads of the calling workgroup, 1024 or 512.  The chunk is written for 16 waves with fixed roles per phase; a 512-thread
// workgroup (two of which share a CU: online_train_kernel's NT = 512 form) runs every phase twice, its wave w taking the roles
// of waves w and w + 8 -- the same SIMD either way, so the per-SIMD MFMA balance of the role tables holds -- and its thread t the
// elements of threads t and t + 512.  Same arithmetic, same sums, whoever executes them.
// SCC = 64 / 128: n_states as a compile-time constant ABOVE 32 (round 5; 0 = any n_states <= 32, a run-time value).  The phases
// that know the state count change shape: a dlogits row is SCC + 2 floats (the arena must have been built with that stride), the
// softmax takes a whole wave per sample (SCC / 64 states per lane), dz2 contracts over SCC / 4 k-steps, and the SCC / 16 x 4 tiles
// of dW3 are looped over by the eight waves that took one each.  1024-thread workgroups only.
// SCC = 256: parameters, gradient and arena together are 210 KB, so W3's gradient (51 KB) has no place in g[] (whose b3 then follows
// b2: kGradW3InRegs below) -- it stays in the MFMA accumulators that compute it.  Its 16 x 4 tiles are dealt four to a wave, wave w
// owning tiles (w >> 2) + 4 j, j = 0..3, of column tile w & 3 (they share the relu(z2) operand), 16 VGPRs `dw3` that the caller keeps
// across the chunks of a pass and hands to apply_dw3_from_regs afterwards.  A chunk adds its tile to the accumulator in the order the
// LDS form adds it to g[] (FIRST: overwrites), one owner per element: the same bits on every run.  The 32 logits tiles go two to a wave.
template <int ROWS, bool FIRST, int NT = kTrainThreads, int SCC = 0, class Hook = NoHook, class Closing = NoHook>
__device__ __forceinline__ void grad_chunk(const float *p, float *g, const TrainLayout &L, const ChunkArena<kTrainChunk> &A, int nc,
                                           float inv_n, int S, Hook idle_hook = Hook(), Closing closing_hook = Closing(),
                                           f32x4 *dw3 = nullptr) {
    constexpr bool first = FIRST;
    constexpr bool BIG = SCC > 32;
    constexpr bool W3REG = SCC > kGradW3InLdsStates;
    constexpr int DLS = BIG ? SCC + 2 : kDlStride;  // floats per dlogits row
    static_assert(!BIG || (NT == kTrainThreads && SCC % 64 == 0), "64, 128 or 256 states on 16 waves");
    static_assert(NT == kTrainThreads || 2 * NT == kTrainThreads, "16 waves, or 8 taking two roles each");
    constexpr int NV = kTrainThreads / NT;  // passes of the physical threads over the 1024 virtual ones
#define MVN_VIRTUAL_WAVES _Pragma("unroll 1") for (int vpass = 0; vpass < NV; ++vpass)
#define MVN_VIRTUAL_IDS const int tid = tid0 + vpass * NT, wave = wave0 + vpass * (NT / 64)
    static_assert(ROWS == 32 || ROWS == 16, "full chunks and 16-row tails");
    constexpr int RT = ROWS / 16;  // 16-row tiles over the samples
    constexpr int AR = kTrainChunk;  // rows of the arena: red[AR ..] hold the running loss and the step sizes
    // the thread index is made opaque here so that the per-lane operand addresses below are recomputed at every call
    // instead of being hoisted out of the step / chunk loops and kept (and spilled) across the whole kernel
    int tid0 = threadIdx.x;
    asm volatile("" : "+v"(tid0));
    const int lane = tid0 & 63;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid0 >> 6);  // 16 (8) waves
    const int li = lane & 15, lq = lane >> 4, rk = rows_k_base<ROWS / 4>(lq);
    const int TS = S > 16 ? S / 16 : 1;  // 16-wide tiles over the states
    float *ys = A.ys, *h1 = A.h1, *z2 = A.z2, *dl = A.dl, *dz2 = A.dz2, *part = A.part, *red = A.red;
    const int *lab = A.lab;
    // ---- forward
    TRAIN_STAMP(0);
    MVN_VIRTUAL_WAVES {  // thread = (unit k = tid % 128, row group tid / 128): its weight and bias once, ROWS / 8 independent sigmoids
        MVN_VIRTUAL_IDS;
        (void)wave;
        const int k = tid & 127, n0 = tid >> 7;
        if (k < kH1 && !MVN_ABL(0)) {
            const float w = p[L.w1 + k], bb = p[L.b1 + k];
            float z[ROWS / 8], h[ROWS / 8];
#pragma unroll
            for (int j = 0; j < ROWS / 8; ++j) z[j] = __builtin_fmaf(ys[n0 + 8 * j], w, bb);
            sigmoid_train_n<ROWS / 8>(z, h);
#pragma unroll
            for (int j = 0; j < ROWS / 8; ++j) h1[(n0 + 8 * j) * kH1Ld + k] = h[j];
        }
    }
    TRAIN_STAMP_WAVE(0);
    __syncthreads();
    TRAIN_STAMP(1);
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    if (tid == kTrainThreads - 1) idle_hook();
    if ((RT == 2 ? wave < 4 : wave < 4) && !MVN_ABL(1)) {  // z2 [ROWS][50] = h1 [ROWS][100] . W2^T: RT x 4 tiles, 25 k-steps
        // one wave per 16 units takes BOTH sample tiles (they share the W2 operand: 3/4 of the LDS bytes of two single tiles, the
        // phase is bound by the operands' LDS bandwidth); every tile accumulates exactly as a single tile does
        const int tn = wave;
        TRAIN_STAMP(16);
        const int m = 16 * tn + li;
        const float bias = p[L.b2 + (m < kH2 ? m : 0)];  // fetched with the operands, not in a round trip of its own afterwards
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RT == 2) {
            const float *const al[2] = {h1 + li * kH1Ld + lq, h1 + (16 + li) * kH1Ld + lq};
            const float *const bl[1] = {p + L.w2 + (16 * tn + li) * kH1Ld + lq};
            f32x4 acc[2][1];
            lds_block_mfma<kK2Steps, 1, 1, false, false, false, 2, 1>(al, bl, acc);
            TRAIN_STAMP(17);
            if (m < kH2)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int r = 0; r < 4; ++r) z2[(16 * tm + 4 * lq + r) * kZ2Stride + m] = acc[tm][0][r] + bias;
        } else {
            const f32x4 acc = lds_tile_mfma<kK2Steps, 1, 1, false, false>(h1 + li * kH1Ld + lq, p + L.w2 + (16 * tn + li) * kH1Ld + lq);
            TRAIN_STAMP(17);
            if (m < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) z2[(4 * lq + r) * kZ2Stride + m] = acc[r] + bias;
        }
        TRAIN_STAMP(18);
    }
    }
    TRAIN_STAMP_WAVE(1);
    __syncthreads();
    TRAIN_STAMP(2);
    if constexpr (W3REG) {  // RT x 16 logits tiles on 16 waves: tiles wave0 and (RT = 2) wave0 + 16
#pragma unroll 1
        for (int t = wave0; t < RT * (SCC / 16); t += kTrainThreads / 64) {
            const int tm = t % RT, ts = t / RT;
            const int s = 16 * ts + li;
            const float bias = p[L.b3 + s];
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 acc = lds_tile_mfma<kK3Steps, 1, 1, true, false>(z2 + (16 * tm + li) * kZ2Stride + lq,
                                                                         p + L.w3 + (16 * ts + li) * kH2 + lq);
#pragma unroll
            for (int r = 0; r < 4; ++r) dl[(16 * tm + 4 * lq + r) * DLS + s] = acc[r] + bias;
        }
    } else
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    (void)tid;
    if (wave < RT * TS && !MVN_ABL(2)) {  // logits [ROWS][S] = relu(z2) [ROWS][50(+2)] . W3^T: RT x TS tiles, 13 k-steps
        const int tm = wave % RT, ts = wave / RT;
        const int s = 16 * ts + li;
        const float bias = p[L.b3 + (s < S ? s : 0)];
        __builtin_amdgcn_sched_barrier(0);
        const f32x4 acc = lds_tile_mfma<kK3Steps, 1, 1, true, false>(z2 + (16 * tm + li) * kZ2Stride + lq,
                                                                     p + L.w3 + (16 * ts + li) * kH2 + lq);
        if (s < S)
#pragma unroll
            for (int r = 0; r < 4; ++r) dl[(16 * tm + 4 * lq + r) * DLS + s] = acc[r] + bias;
    }
    }
    TRAIN_STAMP_WAVE(2);
    __syncthreads();
    TRAIN_STAMP(3);
    // ---- CrossEntropyLoss (mean over the n samples) and its gradient wrt the logits:
    // thread (n, s); the S lanes of a sample are consecutive lanes of one wave (S <= 32)
    if constexpr (BIG) {  // a wave per sample (samples wave, wave + 16), SCC / 64 states per lane; the same sums over the wave's lanes
        const int lane_ = tid0 & 63;
        for (int n = wave0; n < ROWS; n += kTrainThreads / 64) {
            constexpr int NK = SCC / 64;
            float x[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) x[k] = dl[n * DLS + lane_ + 64 * k];
            float mx = x[0];
#pragma unroll
            for (int k = 1; k < NK; ++k) mx = fmaxf(mx, x[k]);
            mx = sample_allreduce<true>(mx, 32);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float sum = 0.0f;
#pragma unroll
            for (int k = 0; k < NK; ++k) sum += expf(x[k] - mx);
            sum = sample_allreduce<false>(sum, 32);
            sum += __shfl_xor(sum, 32);
            const float lg = logf(sum);  // log_softmax = (x - max) - log(sum), torch's order: rounds at |x - max|, not at |max|
            const int label = lab[n];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const bool hit = lane_ + 64 * k == label;
                const float ls = (x[k] - mx) - lg;
                if (hit) red[n] = n < nc ? 0.0f - ls : 0.0f;
                dl[n * DLS + lane_ + 64 * k] = n < nc ? (expf(ls) - (hit ? 1.0f : 0.0f)) * inv_n : 0.0f;
            }
        }
    } else
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    (void)wave;
    if (tid < ROWS * S && !MVN_ABL(3)) {
        const int n = tid / S, s = tid % S;
        const float x = dl[n * DLS + s];
        const float mx = sample_allreduce<true>(x, S);
        const float xm = x - mx;
        const float sum = sample_allreduce<false>(expf(xm), S);
        const float ls = xm - logf(sum);  // log_softmax in torch's order: rounds at |x - max|, not at |max| (DESIGN 5.10.1)
        const bool hit = s == lab[n];
        if (hit) red[n] = n < nc ? 0.0f - ls : 0.0f;
        dl[n * DLS + s] = n < nc ? (expf(ls) - (hit ? 1.0f : 0.0f)) * inv_n : 0.0f;
    }
    }
    TRAIN_STAMP_WAVE(3);
    __syncthreads();
    TRAIN_STAMP(4);
    // ---- backward, output layer: dz2 (first waves), dW3 (waves 8..), db3 and the loss sum (wave 15)
    if (!MVN_ABL(4))
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    (void)tid;
    if (wave < RT * 4) {  // dz2 [ROWS][50] = (dlogits [ROWS][S(+pad)] . W3 [S][50]) * relu'(z2): RT x 4 tiles
        const int tm = wave % RT, tn = wave / RT;
        const float *al = dl + (16 * tm + li) * DLS + lq, *bl = p + L.w3 + lq * kH2 + 16 * tn + li;
        const int k = 16 * tn + li, e0 = (16 * tm + 4 * lq) * kZ2Stride + k;  // (columns 50, 51 hold 0; beyond: the next row)
        float zv[4];  // the mask's z2 values travel with the operands: one LDS round trip less on the phase's critical path
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = z2[e0 + r * kZ2Stride];
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc;
        if constexpr (BIG) acc = lds_tile_mfma<SCC / 4, 1, kH2, false, false>(al, bl);
        else acc = S > 16 ? lds_tile_mfma<8, 1, kH2, false, false>(al, bl) : lds_tile_mfma<4, 1, kH2, false, false>(al, bl);
        if (k < kH2)
#pragma unroll
            for (int r = 0; r < 4; ++r) dz2[e0 + r * kZ2Stride] = zv[r] > 0.0f ? acc[r] : 0.0f;
    } else if (!W3REG && wave >= 8 && wave < 8 + 4 * TS) {  // dW3 [S][50] += dlogits^T [S][ROWS] . relu(z2) [ROWS][50]: TS x 4 tiles
        // (up to 32 states: a tile per wave; SCC: waves 8..15 take tiles wave - 8, wave, wave + 8, ...)
#pragma unroll 1
        for (int t = wave - 8; t < 4 * TS; t += 8) {
            const int ts = t >> 2, tn = t & 3;
            const f32x4 acc = lds_tile_mfma<ROWS / 4, DLS, kZ2Stride, false, true, true>(
                dl + rk * DLS + 16 * ts + li, z2 + rk * kZ2Stride + 16 * tn + li);
            const int k = 16 * tn + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * ts + 4 * lq + r;
                if (s < S && k < kH2) g[L.w3 + s * kH2 + k] = first ? acc[r] : g[L.w3 + s * kH2 + k] + acc[r];
            }
        }
    }
    if constexpr (W3REG) {  // every wave: its four tiles of dW3, into the accumulators (bit for bit the tiles lds_tile_mfma gives)
        const int ts0 = wave >> 2, tn = wave & 3;
        const float *const a0 = dl + rk * DLS + 16 * ts0 + li;
        const float *const al[4] = {a0, a0 + 64, a0 + 128, a0 + 192}, *const bl[1] = {z2 + rk * kZ2Stride + 16 * tn + li};
        f32x4 acc[4][1];
        lds_block_mfma<ROWS / 4, DLS, kZ2Stride, false, true, true, 4, 1>(al, bl, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dw3[j][r] = first ? acc[j][0][r] : dw3[j][r] + acc[j][0][r];
    }
    // db3 (wave 15) and the loss sum (wave 14): 32 operands each, all in flight at once -- one LDS round trip instead of the
    // five the compiler makes of the plain loop (this wave was the last to reach the barrier by 1 000 cycles)
    if (wave == 15 && lane < S) {
#pragma unroll 1
        for (int s = lane; s < S; s += 64) {  // (one trip up to 64 states)
            float dv[ROWS];
#pragma unroll
            for (int n = 0; n < ROWS; ++n) dv[n] = dl[n * DLS + s];
            __builtin_amdgcn_sched_barrier(0);
            float acc = 0.0f;
#pragma unroll
            for (int n = 0; n < ROWS; ++n) acc += dv[n];
            const int e = (W3REG ? L.w3 : L.b3) + s;  // (db3 follows db2 where dW3 is not in g[])
            g[e] = first ? acc : g[e] + acc;
        }
    } else if (wave == 14 && lane == 0) {  // rows n >= nc hold 0
        float rv[ROWS];
#pragma unroll
        for (int n = 0; n < ROWS; ++n) rv[n] = red[n];
        __builtin_amdgcn_sched_barrier(0);
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < ROWS; ++n) acc += rv[n];
        red[AR] += acc;
    }
    }
    TRAIN_STAMP_WAVE(4);
    __syncthreads();
    TRAIN_STAMP(5);
    // ---- backward, hidden layers: RT x 7 tiles of dz1 [ROWS][100] = (dz2 [ROWS][50(+2)] . W2 [50][100]) * h1 (1 - h1)
    // and 28 tiles of dW2 [50][100] += dz2^T [50][ROWS] . h1 [ROWS][100]
    // dz1 = acc * h1 (1 - h1) never goes to memory: its column sums over the tile's 16 rows (db1) and the sums weighted with the
    // inputs (dW1) are all the rest of the pass needs
    auto dz1_epilogue = [&](int tm, int tn, const f32x4 acc) {
        const int k = 16 * tn + li;
        float sb = 0.0f, sw = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = 16 * tm + 4 * lq + r;
            const float h = h1[n * kH1Ld + k];
            const float d = acc[r] * h * (1.0f - h);
            sb += d;
            sw = __builtin_fmaf(d, ys[n], sw);
        }
        sb = sum_over_rows(sb);
        sw = sum_over_rows(sw);
        if (lq == 0) {  // columns k >= 100 of the last tile hold junk: never read
            part[tm * 128 + k] = sb;
            part[(RT + tm) * 128 + k] = sw;
        }
    };
    auto dw2_epilogue = [&](int tm, int tn, const f32x4 acc) {
        const int k = 16 * tn + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * tm + 4 * lq + r;
            if (m < kH2 && k < kH1) g[L.w2 + m * kH1Ld + k] = first ? acc[r] : g[L.w2 + m * kH1Ld + k] + acc[r];
        }
    };
    // The phase is bound by the SIMDs' MFMA time (an f32 MFMA holds its SIMD for ~35 cycles and excludes everything else there,
    // DESIGN 5.0), then by the LDS bytes of the operands.  So (a) no MFMA is spent on padding: units 48, 49 of dW2 would cost a
    // fourth row tile (7 tiles x 8 MFMAs for 2 of 16 rows) and go to the vector ALU -- after this phase, because while the tile
    // products keep the LDS queue full a chain of LDS round trips takes ~500 cycles per link (a wave doing them here, even at
    // raised priority, reached the barrier 2 500 cycles after everyone else); (b) tiles are taken in blocks that share operands;
    // (c) the blocks are dealt so that every SIMD (wave w runs on SIMD w % 4) gets the same MFMA count within 10 %:
    // 84 / 92 / 90 / 84 of 350.
    //   wave  0  1  2 : dW2 units 0..31  x inputs 32 w .. 32 w + 31   (2 x 2 tiles, 32 MFMAs)
    //   wave  3       : dW2 units 0..31  x inputs 96..99              (2 x 1, 16)
    //   wave 10 14 15 : dW2 units 32..47 x inputs 0..31, 32..63, 64..95   (1 x 2, 16)
    //   wave 13       : dW2 units 32..47 x inputs 96..99              (1 x 1, 8)
    //   wave 4..9, 11 : dz1 input tile 0, 2, 4, 5, 1, 3, 6 for both sample tiles (2 x 1 sharing W2's columns, 26)
    //   wave 12       : nothing
    const float *const dz2_rows = dz2 + rk * kZ2Stride + li, *const h1_rows = h1 + rk * kH1Ld + li;
    if (!MVN_ABL(5))
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    (void)tid;
    if constexpr (RT == 1) {
        // 16 rows: 7 dz1 tiles of 13 MFMAs and 21 dW2 tiles of 4 (the contraction over 16 samples); per SIMD 50 / 50 / 38 / 37
        //   wave 0..6  : dz1 input tile w
        //   wave 7     : dW2 units 0..47 x inputs 96..99          (3 x 1 tiles sharing h1's columns, 12 MFMAs)
        //   wave 8..13 : dW2 units 0..47 x inputs 16 (w - 8) ..   (3 x 1, 12)
        if (wave < 7) {
            dz1_epilogue(0, wave, lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(dz2 + li * kZ2Stride + lq,
                                                                                  p + L.w2 + lq * kH1Ld + 16 * wave + li));
        } else if (wave < 14) {
            const int tn = wave == 7 ? 6 : wave - 8;
            const float *const al[3] = {dz2_rows, dz2_rows + 16, dz2_rows + 32}, *const bl[1] = {h1_rows + 16 * tn};
            f32x4 acc[3][1];
            lds_block_mfma<ROWS / 4, kZ2Stride, kH1Ld, false, false, true, 3, 1>(al, bl, acc);
            dw2_epilogue(0, tn, acc[0][0]);
            dw2_epilogue(1, tn, acc[1][0]);
            dw2_epilogue(2, tn, acc[2][0]);
        }
    } else if (wave < 3) {
        TRAIN_STAMP(10);
        const float *const al[2] = {dz2_rows, dz2_rows + 16}, *const bl[2] = {h1_rows + 32 * wave, h1_rows + 32 * wave + 16};
        f32x4 acc[2][2];
        lds_block_mfma<ROWS / 4, kZ2Stride, kH1Ld, false, false, true, 2, 2>(al, bl, acc);
        TRAIN_STAMP(11);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) dw2_epilogue(i, 2 * wave + j, acc[i][j]);
        TRAIN_STAMP(12);
    } else if (wave == 3) {
        const float *const al[2] = {dz2_rows, dz2_rows + 16}, *const bl[1] = {h1_rows + 96};
        f32x4 acc[2][1];
        lds_block_mfma<ROWS / 4, kZ2Stride, kH1Ld, false, false, true, 2, 1>(al, bl, acc);
        dw2_epilogue(0, 6, acc[0][0]);
        dw2_epilogue(1, 6, acc[1][0]);
    } else if (wave == 10 || wave >= 14) {
        const int tn0 = wave == 10 ? 0 : wave == 14 ? 2 : 4;
        const float *const al[1] = {dz2_rows + 32}, *const bl[2] = {h1_rows + 16 * tn0, h1_rows + 16 * tn0 + 16};
        f32x4 acc[1][2];
        lds_block_mfma<ROWS / 4, kZ2Stride, kH1Ld, false, false, true, 1, 2>(al, bl, acc);
        dw2_epilogue(2, tn0, acc[0][0]);
        dw2_epilogue(2, tn0 + 1, acc[0][1]);
    } else if (wave == 13) {
        dw2_epilogue(2, 6, lds_tile_mfma<ROWS / 4, kZ2Stride, kH1Ld, false, false, true>(dz2_rows + 32, h1_rows + 96));
    } else if (wave != 12) {
        const int tn = wave == 4 ? 0 : wave == 5 ? 2 : wave == 6 ? 4 : wave == 7 ? 5 : wave == 8 ? 1 : wave == 9 ? 3 : 6;
        const float *const al[2] = {dz2 + li * kZ2Stride + lq, dz2 + (16 + li) * kZ2Stride + lq};
        const float *const bl[1] = {p + L.w2 + lq * kH1Ld + 16 * tn + li};
        f32x4 acc[2][1];
        lds_block_mfma<kK3Steps, 1, kH1Ld, false, false, false, 2, 1>(al, bl, acc);
        dz1_epilogue(0, tn, acc[0][0]);
        dz1_epilogue(1, tn, acc[1][0]);
    }
    }
    TRAIN_STAMP(14);
    TRAIN_STAMP_WAVE(5);
    __syncthreads();
    TRAIN_STAMP(6);
    // What is left, with the LDS quiet (one round trip each):
    // * dW1 [100], db1 [100] from the column sums: thread t < 50, one 16-byte read-modify-write (L.w1 = 0, L.b1 = 100: float4 t
    //   of g is w1 or b1 [4 t' ..])
    // * dW2 units 48, 49 (waves 4..7: unit 48 + (wave - 4) / 2, input k = lane of the wave pair): 32 products in sample order
    // * db2 (wave 8)
    if (!MVN_ABL(6))
    MVN_VIRTUAL_WAVES {
    MVN_VIRTUAL_IDS;
    if (tid < 2 * kH1 / 4) {
        const int t4 = tid < kH1 / 4 ? tid : tid - kH1 / 4;
        const float4 *src = reinterpret_cast<const float4 *>(part + (tid < kH1 / 4 ? RT * 128 : 0)) + t4;
        float4 acc = src[0];
        if (RT > 1) {
            const float4 o = src[128 / 4];
            acc = make_float4(acc.x + o.x, acc.y + o.y, acc.z + o.z, acc.w + o.w);
        }
        float4 *dst = reinterpret_cast<float4 *>(g) + tid;
        if (!first) {
            const float4 gv = *dst;
            acc = make_float4(gv.x + acc.x, gv.y + acc.y, gv.z + acc.z, gv.w + acc.w);
        }
        *dst = acc;
    } else if (wave >= 4 && wave < 8) {
        const int unit = 48 + ((wave - 4) >> 1), k = tid & 127;
        if (k < kH1) {  // all 64 operands in flight at once (left alone the compiler takes them in eight round trips)
            float dv[ROWS], hv[ROWS];
#pragma unroll
            for (int n = 0; n < ROWS; ++n) {
                dv[n] = dz2[n * kZ2Stride + unit];
                hv[n] = h1[n * kH1Ld + k];
            }
            __builtin_amdgcn_sched_barrier(0);
            float acc = 0.0f;
#pragma unroll
            for (int n = 0; n < ROWS; ++n) acc = __builtin_fmaf(dv[n], hv[n], acc);
            g[L.w2 + unit * kH1Ld + k] = first ? acc : g[L.w2 + unit * kH1Ld + k] + acc;
        }
    } else if (wave == 8 && lane < kH2) {
        float dv[ROWS];
#pragma unroll
        for (int n = 0; n < ROWS; ++n) dv[n] = dz2[n * kZ2Stride + lane];
        __builtin_amdgcn_sched_barrier(0);
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < ROWS; ++n) acc += dv[n];
        g[L.b2 + lane] = first ? acc : g[L.b2 + lane] + acc;
    }
    }
    closing_hook();
    TRAIN_STAMP_WAVE(6);
    __syncthreads();
    TRAIN_STAMP(7);
#undef MVN_VIRTUAL_WAVES
#undef MVN_VIRTUAL_IDS
}

// torch.optim.Adam update (amsgrad=False, weight_decay=0) of one parameter.  denom = sqrt(v) / sqrt(1 - beta2^t) + eps and
// m / denom use v_sqrt_f32 / v_rcp_f32 (1 ulp each) and the reciprocal of the bias correction (the IEEE sqrt and two
// divisions were a quarter of an iteration).
// The trainer's other two optimizers (deep_learning_setup, trainer.py:163-175: torch.optim.RMSprop / SGD with torch's defaults --
// no momentum, no weight decay, not centered) ride on the same entry points: beta1 < 0 selects them (MVN_BETA1_RMSPROP = -1 with
// alpha = beta2, MVN_BETA1_SGD = -2; include/mvn.h), launch-uniform, and step_size is then the plain learning rate
// (train_step_size below).  RMSprop keeps its square average in v (exp_avg_sq), m is left alone; SGD touches neither.
__device__ __forceinline__ void adam1(float &p, float &m, float &v, float gr, float beta1, float beta2, float eps,
                                      float step_size, float inv_sqrt_bc2) {
    if (beta1 >= 0.0f) {
        m = beta1 * m + (1.0f - beta1) * gr;
        v = beta2 * v + (1.0f - beta2) * gr * gr;
        const float denom = __builtin_amdgcn_sqrtf(v) * inv_sqrt_bc2 + eps;
        p = p - step_size * (m * __builtin_amdgcn_rcpf(denom));
    } else if (beta1 > -1.5f) {  // RMSprop: square_avg = alpha square_avg + (1 - alpha) g^2; p -= lr g / (sqrt(square_avg) + eps)
        v = beta2 * v + (1.0f - beta2) * gr * gr;
        p = p - step_size * (gr * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + eps));
    } else {  // SGD: p -= lr g
        p = p - step_size * gr;
    }
}
// the step size of an iteration: Adam's lr / (1 - beta1^t), in double like torch's Python side; the plain lr for RMSprop / SGD
__device__ __forceinline__ float train_step_size(float lr, float beta1, double b1pow) {
    return beta1 >= 0.0f ? (float)((double)lr / (1.0 - b1pow)) : lr;
}
__device__ __forceinline__ void adam4(float4 &p4, float4 &m4, float4 &v4, const float4 gr4, float beta1, float beta2,
                                      float eps, float step_size, float inv_sqrt_bc2) {
    adam1(p4.x, m4.x, v4.x, gr4.x, beta1, beta2, eps, step_size, inv_sqrt_bc2);
    adam1(p4.y, m4.y, v4.y, gr4.y, beta1, beta2, eps, step_size, inv_sqrt_bc2);
    adam1(p4.z, m4.z, v4.z, gr4.z, beta1, beta2, eps, step_size, inv_sqrt_bc2);
    adam1(p4.w, m4.w, v4.w, gr4.w, beta1, beta2, eps, step_size, inv_sqrt_bc2);
}

// The optimizer step of W3 at 256 states, from the accumulators grad_chunk left its gradient in: lane (li, lq) of wave w holds
// dW3[16 ((w >> 2) + 4 j) + 4 lq + r][16 (w & 3) + li] in dw3[j][r] (the MFMA's output layout).  W3 is in LDS, its moments are
// elements w3_flat + s * 50 + k of the flat vectors in global memory; the same adam1 per element as everywhere else.
__device__ __forceinline__ void apply_dw3_from_regs(float *p, const TrainLayout &L, const f32x4 *dw3, float *__restrict__ adam_m,
                                                    float *__restrict__ adam_v, float beta1, float beta2, float eps, float step_size,
                                                    float inv_sqrt_bc2) {
    // (the thread index is made opaque, as in grad_chunk: the 48 element offsets below are then recomputed in every iteration; left
    // alone they are hoisted out of the iteration loop, spilled, and reloaded from scratch here each time)
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    const int lane = t & 63, wave = t >> 6, li = lane & 15, lq = lane >> 4;
    const int k = 16 * (wave & 3) + li, w3_flat = L.w3 - kH2 * (kH1Ld - kH1);
    const bool live = k < kH2;  // (the fourth column tile holds units 48, 49 only; its other lanes load element 0 and store nothing)
#pragma unroll
    for (int j0 = 0; j0 < 4; j0 += 2) {  // two tiles at a time: 16 global loads in flight together (all four: the registers spill)
        float me[2][4], ve[2][4], pe[2][4];
        unsigned o[2][4];  // (unsigned: a 32-bit offset from the uniform base pointer, no 64-bit address per load)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[j][r] = live ? (unsigned)((16 * ((wave >> 2) + 4 * (j0 + j)) + 4 * lq + r) * kH2 + k) : 0u;
                me[j][r] = adam_m[(unsigned)w3_flat + o[j][r]];
                ve[j][r] = adam_v[(unsigned)w3_flat + o[j][r]];
                pe[j][r] = p[(unsigned)L.w3 + o[j][r]];
            }
        __builtin_amdgcn_sched_barrier(0);
        if (live)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    adam1(pe[j][r], me[j][r], ve[j][r], dw3[j0 + j][r], beta1, beta2, eps, step_size, inv_sqrt_bc2);
                    p[(unsigned)L.w3 + o[j][r]] = pe[j][r];
                    adam_m[(unsigned)w3_flat + o[j][r]] = me[j][r];
                    adam_v[(unsigned)w3_flat + o[j][r]] = ve[j][r];
                }
    }
}

// Staging of a trial's six parameter arrays (torch layout, six separate pointers) into / out of the LDS vector
template <int NT = kTrainThreads>
__device__ __forceinline__ void load_params(float *p, const TrainLayout &L, int S, const float *const (&src)[6]) {
    const int off[6] = {L.w1, L.b1, L.w2, L.b2, L.w3, L.b3};
    const int len[6] = {kH1, kH1, kH2 * kH1, kH2, S * kH2, S};  // global (unpadded) lengths
#pragma unroll
    for (int a = 0; a < 6; ++a)
        for (int e = threadIdx.x; e < len[a]; e += NT) p[off[a] + (a == 2 ? (e / kH1) * kH1Ld + e % kH1 : e)] = src[a][e];
}
template <int NT = kTrainThreads>
__device__ __forceinline__ void store_params(const float *p, const TrainLayout &L, int S, float *const (&dst)[6]) {
    const int off[6] = {L.w1, L.b1, L.w2, L.b2, L.w3, L.b3};
    const int len[6] = {kH1, kH1, kH2 * kH1, kH2, S * kH2, S};
#pragma unroll
    for (int a = 0; a < 6; ++a)
        for (int e = threadIdx.x; e < len[a]; e += NT) dst[a][e] = p[off[a] + (a == 2 ? (e / kH1) * kH1Ld + e % kH1 : e)];
}
// a trial's result: w_out, and w_out2 when given (the evaluation's saved detector, trainer.py:343)
template <int NT = kTrainThreads>
__device__ __forceinline__ void store_trial_params(const float *p, const TrainLayout &L, int S, const mvn_train_trial_t &d) {
    store_params<NT>(p, L, S, d.w_out);
    if (d.w_out2[0]) store_params<NT>(p, L, S, d.w_out2);
}

// ---- the frame the training kernels share around grad_chunk / hv_chunk.  A piece is shared only in a form that leaves the disassembly
// of every training kernel as it was (tools/kernel_isa_diff.py): a function where that holds, else a text, and what changes code
// either way stays duplicated (the clear_pads_* lambdas of the meta-learning kernels; profiles/train_isa_identity.txt).
// Every float the tile products can touch must be finite: clear the whole allocation first (padding columns and the operand rows
// read past a matrix edge stay zero or hold live finite data afterwards), then stage the parameters `p` of trial `d`.
// (A text: as a function it changes maml_train_kernel.)
#define MVN_CLEAR_LDS_LOAD_PARAMS(NT, p)                           \
    do {                                                           \
        for (int e = tid; e < lds_floats; e += NT) smem[e] = 0.0f; \
        __syncthreads();                                           \
        load_params<NT>(p, L, S, d.w_in);                          \
    } while (0)

// Adam's moments (flat torch order in global memory) into / out of the LDS vectors
template <int NT = kTrainThreads>
__device__ __forceinline__ void moments_to_lds(float *am, float *av, const float *adam_m, const float *adam_v, int Pflat, int tid) {
    for (int e = tid; e < Pflat; e += NT) {
        am[lds_index(e)] = adam_m[e];
        av[lds_index(e)] = adam_v[e];
    }
}
template <int NT = kTrainThreads>
__device__ __forceinline__ void moments_from_lds(const float *am, const float *av, float *adam_m, float *adam_v, int Pflat, int tid) {
    for (int e = tid; e < Pflat; e += NT) {
        adam_m[e] = am[lds_index(e)];
        adam_v[e] = av[lds_index(e)];
    }
}

// Adam's bias corrections of the next step, in double like torch's Python side: advances the running powers.  ADAM_ONLY: the
// meta-learning kernels (their entry points refuse the RMSprop / SGD tags) spell the step size out.
template <bool ADAM_ONLY>
__device__ __forceinline__ void next_bias_corrections(double &b1pow, double &b2pow, float lr, float beta1, float beta2, float &step_size,
                                                      float &inv_sqrt_bc2) {
    b1pow *= (double)beta1;
    b2pow *= (double)beta2;
    step_size = ADAM_ONLY ? (float)((double)lr / (1.0 - b1pow)) : train_step_size(lr, beta1, b1pow);
    inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - b2pow));
}

// SC: n_states as a compile-time constant (16, 32: every LDS offset becomes an immediate) or 0 = run-time S_rt (any S <= 32).
// MANY = false: the trial is the by-value argument `one` (the single-trial entry points); true: trial blockIdx.y of the
// device array `many` (mvn_vnet_online_train_trials_f32), a trial with n = 0 exits at once.
// NT = 1024: one workgroup per CU (parameters, gradient, both Adam moments and the chunk images: 141 KB of LDS at 16 states).
// NT = 512: the form for MORE TRIALS THAN CUs -- parameters, gradient and a compact chunk arena are 79.3 KB, so TWO workgroups
// share a CU and one's barrier waits, LDS round trips and half-empty phases are filled by the other's work (the chunk phases
// leave the SIMDs' pipes idle ~40 % of the time, profiles/r04_train_pmc.csv); every wave takes two of the 16 roles per phase
// (grad_chunk, NT), and Adam's moments stay in global memory (48 KB per trial: L2-resident), read and written once per
// iteration.  Same arithmetic as the 1024-thread form: bit-identical results.
template <int SC, bool MANY, int NT = kTrainThreads>
__global__ __launch_bounds__(NT, NT == kTrainThreads ? 1 : 4) void online_train_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int M, float lr, float beta1, float beta2,
    float eps, int S_rt, int lds_floats) {
#define MVN_TRAIN_WORDS 0
#include "online_train_body.inc"
#undef MVN_TRAIN_WORDS
}

// The word axis (mvn_vnet_train_words_f32): one trial, one 1024-thread workgroup, every state count online_train_kernel<SC, false>
// serves, the same body with the word fetched beside the sample index.  T: the labelled positions of a word (T <= ld_y, T <= ld_lab;
// an iteration's samples are drawn from [0, T), or are all T).  `many` is unused (the launcher's argument frame).
template <int SC>
__global__ __launch_bounds__(kTrainThreads, 1) void online_train_words_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int M, int ld_y, int ld_lab, float lr, float beta1,
    float beta2, float eps, int S_rt, int lds_floats) {
    constexpr bool MANY = false;
    constexpr int NT = kTrainThreads;
#define MVN_TRAIN_WORDS 1
#include "online_train_body.inc"
#undef MVN_TRAIN_WORDS
}

// 256 states on the word axis.  Its own name, not online_train_words_kernel<256>: that template's instantiations are the five
// state constants the trial axis shares, and this form has no trial-batched twin.
__global__ __launch_bounds__(kTrainThreads, 1) void online_train_words_states256_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int M, int ld_y, int ld_lab, float lr, float beta1,
    float beta2, float eps, int S_rt, int lds_floats) {
    constexpr int SC = 256;
    constexpr bool MANY = false;
    constexpr int NT = kTrainThreads;
#define MVN_TRAIN_WORDS 1
#include "online_train_body.inc"
#undef MVN_TRAIN_WORDS
}

inline size_t online_train_lds_floats(int S) {
    const TrainLayout L = train_layout(S);
    // + 64: operand rows read past the last activation image (discarded output columns) stay inside the allocation
    // 256 states: the gradient vector without dW3 (registers: grad_chunk) -- 158 668 bytes of the CU's 163 840
    if (S > kGradW3InLdsStates) return (size_t)2 * L.P4 - (size_t)S * kH2 + ChunkArena<kTrainChunk>::floats(S + 2) + 64;
    if (S > 32) return (size_t)2 * L.P4 + ChunkArena<kTrainChunk>::floats(S + 2) + 64;  // (moments in global memory)
    return (size_t)4 * L.P4 + ChunkArena<kTrainChunk>::kFloats + 64;
}
inline size_t online_train_lds_bytes(int S) { return online_train_lds_floats(S) * sizeof(float); }
// the 512-thread form: parameters, gradient, compact arena (must stay within half a CU's 160 KB)
constexpr int kTrainThreads2 = kTrainThreads / 2;
inline size_t online_train2_lds_floats(int S) {
    const TrainLayout L = train_layout(S);
    return (size_t)2 * L.P4 + ChunkArena<kTrainChunk>::kFloatsCompact + 64;
}
inline size_t online_train2_lds_bytes(int S) { return online_train2_lds_floats(S) * sizeof(float); }
