// maml_train.inc -- the online meta-learning step of Meta-ViterbiNet as one persistent workgroup (SURVEY 8f next #3),
// included by mvn_hip.hip after online_train.inc, whose parameter layout, LDS tile products, chunk gradient and Adam
// update it reuses.
//
// Counterpart of Trainer.meta_train_loop (python_code/trainers/trainer.py:425-453) with METAVNETTrainer.calc_loss
// (trainers/META_VNET/metavnet_trainer.py:41-50), n_steps times in ONE launch:
//     g_s   = grad L_support(theta)                         (CrossEntropy over the support words' symbols)
//     theta' = theta - meta_lr * g_s                        (inner SGD step, trainer.py:437-440)
//     g_q   = grad L_query(theta')
//     meta  = g_q - meta_lr * H_support(theta) g_q          (second order, MAML; first order: meta = g_q)
//     theta <- Adam(theta, meta)                            (the trainer's single optimizer, :452)
// The reference gets the second-order term from autograd (create_graph=True, ~200 ATen kernels per step).  Here the
// Hessian-vector product is the directional derivative of the support gradient along v = g_q (Pearlmutter's R-operator),
// written out for this network (z1 = w1 y + b1, h1 = sigmoid(z1), z2 = W2 h1 + b2, a2 = relu(z2), o = W3 a2 + b3,
// p = softmax(o), do = (p - onehot) / n) with s' = h1 (1 - h1) and R(.) the tangent of a quantity:
//     R z1 = vw1 y + vb1            R h1 = s' R z1
//     R z2 = W2 R h1 + vW2 h1 + vb2           R a2 = R z2 [z2 > 0]
//     R o  = W3 R a2 + vW3 a2 + vb3           R do = p (R o - <p, R o>) / n
//     R dW3 = R do a2^T + do R a2^T           R db3 = sum R do
//     R dz2 = (W3^T R do + vW3^T do) [z2 > 0]
//     R dW2 = R dz2 h1^T + dz2 R h1^T         R db2 = sum R dz2
//     R dz1 = (W2^T R dz2 + vW2^T dz2) s' + (W2^T dz2) s' (1 - 2 h1) R z1
//     R dw1 = sum R dz1 y                     R db1 = sum R dz1
// (checked against torch's double backward to 1e-16 in float64 before it was written; tests/ compare the kernel with
// meta.meta_train_loop).  Every product is a 16x16 MFMA tile fed from LDS as in online_train.inc; the Hessian pass works
// on 32-sample chunks whose primal and tangent images take the place of theta' (dead by then) and of the gradient passes' arena,
// next to theta and the two accumulators in the 160 KB of LDS; Adam's moments stay in global memory (touched once per step).
// That is the layout up to 32 states; at 64 and 128 states two vectors and 16-sample Hessian chunks do (the end of this file).
// Samples per chunk of the Hessian pass.  32 like the gradient passes: a 16-sample chunk costs 70 % of a 32-sample one (barriers,
// LDS round trips and half-empty phases do not shrink with the rows).  Its images need 68 KB next to theta and the two accumulators;
// they start where theta' lives, which is dead by then (hv_chunk<16> is kept instantiable: tests of the tile dealing).
constexpr int kHvRows = 32;

template <int R>
struct HvArena {  // LDS images of one R-sample chunk of the Hessian pass (aliases the gradient passes' ChunkArena)
    float *ys;    // [R]
    int *lab;     // [R]
    float *h1;    // [R][100]
    float *Rh1;   // [R][100]
    float *z2;    // [R][52]
    float *Ra2;   // [R][52]  R z2, then masked
    float *pr;    // [R][dls] logits, then probabilities (dls: kDlStride up to 32 states, n_states + 2 above, as ChunkArena)
    float *dlo;   // [R][dls] do
    float *Rdo;   // [R][dls] R o, then R do
    float *dz2;   // [R][52]
    float *Rdz2;  // [R][52]
    float *part;  // [2][R / 16][128]: per 16-row tile, column sums of R dz1 (-> R db1) and of R dz1 * y (-> R dW1)
    static constexpr int floats(int dls) { return 2 * R + R * (2 * kH1Ld + 4 * kZ2Stride + 3 * dls) + 2 * (R / 16) * 128; }
    static constexpr int kFloats = floats(kDlStride);
    __device__ explicit HvArena(float *base, int dls = kDlStride) {
        ys = base;
        lab = (int *)(ys + R);
        h1 = ys + 2 * R;
        Rh1 = h1 + R * kH1Ld;
        z2 = Rh1 + R * kH1Ld;
        Ra2 = z2 + R * kZ2Stride;
        pr = Ra2 + R * kZ2Stride;
        dlo = pr + R * dls;
        Rdo = dlo + R * dls;
        dz2 = Rdo + R * dls;
        Rdz2 = dz2 + R * kZ2Stride;
        part = Rdz2 + R * kZ2Stride;
    }
};

__device__ __forceinline__ f32x4 f4add(f32x4 a, f32x4 b) { return f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]}; }

// Adds the chunk's share of H_support(theta) v to hv[]: p = theta, v = the direction (both TrainLayout vectors in LDS),
// A.ys / A.lab in place, inv_n = 1 / (support samples), rows >= nc are padding.  All threads call it; ends with a barrier.
// R = 16 or 32 samples (RT = R / 16 row tiles): the tile products of a phase are numbered and dealt to the 16 waves in turn; with
// 16 samples every wave gets at most one per phase except in the last (R dz1 / R dW2: 35 products).
// (R = 16 with the 32-row arena: a chunk whose samples all sit in rows 0..15, like grad_chunk<16>)
template <int R>
__device__ __forceinline__ void hv_chunk(const float *p, const float *v, float *hv, const TrainLayout &L, const HvArena<kHvRows> &A,
                                         int nc, float inv_n, int S) {
    constexpr int RT = R / 16, kWaves = kTrainThreads / 64;
    // the thread index is made opaque here so that the per-lane operand addresses below are recomputed at every call
    // instead of being hoisted out of the step / chunk loops and kept (and spilled) across the whole kernel
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4, rk = rows_k_base<R / 4>(lq);
    const int TS = S > 16 ? S / 16 : 1;
    // ---- layer 1 and its tangent
    for (int e = tid; e < R * kH1; e += kTrainThreads) {
        const int n = e / kH1, k = e % kH1;
        const float h = sigmoid_train(__builtin_fmaf(A.ys[n], p[L.w1 + k], p[L.b1 + k]));
        A.h1[n * kH1Ld + k] = h;
        A.Rh1[n * kH1Ld + k] = h * (1.0f - h) * __builtin_fmaf(A.ys[n], v[L.w1 + k], v[L.b1 + k]);
    }
    __syncthreads();
    // ---- z2 (products 0 .. 4 RT - 1) and R z2 = W2 R h1 + vW2 h1 + vb2 (4 RT .. 8 RT - 1): RT x 4 tiles of 16 units each
    for (int job = wave; job < 8 * RT; job += kWaves) {
        const bool tangent = job >= 4 * RT;
        const int j = tangent ? job - 4 * RT : job, tm = j % RT, tn = j / RT, m = 16 * tn + li, row = 16 * tm + li;
        // (biases fetched with the operands, not in an LDS round trip of their own after the products: as in grad_chunk)
        const float bias = (tangent ? v : p)[L.b2 + (m < kH2 ? m : 0)];
        __builtin_amdgcn_sched_barrier(0);
        if (!tangent) {
            const f32x4 acc = lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.h1 + row * kH1Ld + lq, p + L.w2 + m * kH1Ld + lq);
            if (m < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.z2[(16 * tm + 4 * lq + r) * kZ2Stride + m] = acc[r] + bias;
        } else {
            const f32x4 acc = f4add(lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.Rh1 + row * kH1Ld + lq, p + L.w2 + m * kH1Ld + lq),
                                    lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.h1 + row * kH1Ld + lq, v + L.w2 + m * kH1Ld + lq));
            if (m < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.Ra2[(16 * tm + 4 * lq + r) * kZ2Stride + m] = acc[r] + bias;
        }
    }
    __syncthreads();
    for (int e = tid; e < R * kH2; e += kTrainThreads) {  // R a2 = R z2 [z2 > 0]
        const int i = (e / kH2) * kZ2Stride + e % kH2;
        A.Ra2[i] = A.z2[i] > 0.0f ? A.Ra2[i] : 0.0f;
    }
    __syncthreads();
    // ---- logits (products 0 .. RT TS - 1) and R o = W3 R a2 + vW3 a2 + vb3 (RT TS .. 2 RT TS - 1)
    for (int job = wave; job < 2 * RT * TS; job += kWaves) {
        const bool tangent = job >= RT * TS;
        const int j = tangent ? job - RT * TS : job, tm = j % RT, s = 16 * (j / RT) + li, row = 16 * tm + li;
        const float bias = (tangent ? v : p)[L.b3 + (s < S ? s : 0)];
        __builtin_amdgcn_sched_barrier(0);
        if (!tangent) {
            const f32x4 acc = lds_tile_mfma<kK3Steps, 1, 1, true, false>(A.z2 + row * kZ2Stride + lq, p + L.w3 + s * kH2 + lq);
            if (s < S)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.pr[(16 * tm + 4 * lq + r) * kDlStride + s] = acc[r] + bias;
        } else {
            const f32x4 acc = f4add(lds_tile_mfma<kK3Steps, 1, 1, false, false>(A.Ra2 + row * kZ2Stride + lq, p + L.w3 + s * kH2 + lq),
                                    lds_tile_mfma<kK3Steps, 1, 1, true, false>(A.z2 + row * kZ2Stride + lq, v + L.w3 + s * kH2 + lq));
            if (s < S)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.Rdo[(16 * tm + 4 * lq + r) * kDlStride + s] = acc[r] + bias;
        }
    }
    __syncthreads();
    // ---- softmax, do and R do = p (R o - <p, R o>) / n: thread (n, s), the S lanes of a sample adjacent in one wave
    if (tid < R * S) {
        const int n = tid / S, s = tid % S;
        const float x = A.pr[n * kDlStride + s];
        const float mx = sample_allreduce<true>(x, S);
        const float sum = sample_allreduce<false>(expf(x - mx), S);
        const float prob = expf((x - mx) - logf(sum));  // torch's log_softmax order: rounds at |x - max|, not at |max| (DESIGN 5.10.1)
        const float ro = A.Rdo[n * kDlStride + s];
        const float dot = sample_allreduce<false>(prob * ro, S);
        const bool live = n < nc;
        A.dlo[n * kDlStride + s] = live ? (prob - (s == A.lab[n] ? 1.0f : 0.0f)) * inv_n : 0.0f;
        A.Rdo[n * kDlStride + s] = live ? prob * (ro - dot) * inv_n : 0.0f;
    }
    __syncthreads();
    // ---- dz2 (products 0 .. 4 RT - 1), R dz2 = (W3^T R do + vW3^T do) [z2 > 0] (4 RT .. 8 RT - 1), R dW3 (the next 4 TS);
    // R db3 by wave 15
    for (int job = wave; job < 8 * RT + 4 * TS; job += kWaves) {
        if (job < 8 * RT) {
            const bool tangent = job >= 4 * RT;
            const int j = tangent ? job - 4 * RT : job, tm = j % RT, tn = j / RT, k = 16 * tn + li, row = 16 * tm + li;
            const float *dl_l = A.dlo + row * kDlStride + lq, *rd_l = A.Rdo + row * kDlStride + lq;
            const float *w3p = p + L.w3 + lq * kH2 + k, *w3v = v + L.w3 + lq * kH2 + k;
            const int e0 = (16 * tm + 4 * lq) * kZ2Stride + k;
            float zv[4];  // the mask's z2 values travel with the operands
#pragma unroll
            for (int r = 0; r < 4; ++r) zv[r] = A.z2[e0 + r * kZ2Stride];
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc;
            if (!tangent) {
                acc = S > 16 ? lds_tile_mfma<8, 1, kH2, false, false>(dl_l, w3p) : lds_tile_mfma<4, 1, kH2, false, false>(dl_l, w3p);
            } else {
                acc = S > 16 ? f4add(lds_tile_mfma<8, 1, kH2, false, false>(rd_l, w3p), lds_tile_mfma<8, 1, kH2, false, false>(dl_l, w3v))
                             : f4add(lds_tile_mfma<4, 1, kH2, false, false>(rd_l, w3p), lds_tile_mfma<4, 1, kH2, false, false>(dl_l, w3v));
            }
            // (base + offset, not a choice between two pointers: that loses the LDS address space and the stores become flat
            // ones -- the Hessian pass ran 18 % slower)
            float *dst = A.dz2 + (tangent ? kHvRows * kZ2Stride : 0);  // R dz2 follows dz2 in the (32-row) arena
            if (k < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[e0 + r * kZ2Stride] = zv[r] > 0.0f ? acc[r] : 0.0f;
        } else {  // R dW3 [S][50] = R do^T a2 + do^T R a2, contraction over the R samples
            const int j = job - 8 * RT, ts = j >> 2, tn = j & 3, k = 16 * tn + li;
            const f32x4 acc = f4add(lds_tile_mfma<R / 4, kDlStride, kZ2Stride, false, true, true>(A.Rdo + rk * kDlStride + 16 * ts + li,
                                                                                                 A.z2 + rk * kZ2Stride + k),
                                    lds_tile_mfma<R / 4, kDlStride, kZ2Stride, false, false, true>(A.dlo + rk * kDlStride + 16 * ts + li,
                                                                                                  A.Ra2 + rk * kZ2Stride + k));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = 16 * ts + 4 * lq + r;
                if (s < S && k < kH2) hv[L.w3 + s * kH2 + k] += acc[r];
            }
        }
    }
    if (wave == 15 && lane < S) {  // all R operands in one LDS round trip (as grad_chunk's db3)
        float dv[R];
#pragma unroll
        for (int n = 0; n < R; ++n) dv[n] = A.Rdo[n * kDlStride + lane];
        __builtin_amdgcn_sched_barrier(0);
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < R; ++n) acc += dv[n];
        hv[L.b3 + lane] += acc;
    }
    __syncthreads();
    // ---- 7 RT tiles of R dz1 (products 0 ..) and 28 tiles of R dW2 = R dz2^T h1 + dz2^T R h1; R db2
    for (int job = wave; job < 7 * RT + 28; job += kWaves) {
        if (job < 7 * RT) {
            const int tm = job % RT, k = 16 * (job / RT) + li, row = 16 * tm + li;
            const float *w2p = p + L.w2 + lq * kH1Ld + k, *w2v = v + L.w2 + lq * kH1Ld + k;
            const f32x4 dh1 = lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.dz2 + row * kZ2Stride + lq, w2p);
            const f32x4 rdh1 = f4add(lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.Rdz2 + row * kZ2Stride + lq, w2p),
                                     lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.dz2 + row * kZ2Stride + lq, w2v));
            // R dz1 stays in registers: only its column sums over the tile's 16 rows (R db1) and the sums weighted with the
            // inputs (R dW1) are needed (as in grad_chunk)
            float sb = 0.0f, sw = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = 16 * tm + 4 * lq + r, e = n * kH1Ld + k;
                const float h = A.h1[e], sp = h * (1.0f - h);
                const float rz1 = __builtin_fmaf(A.ys[n], v[L.w1 + k], v[L.b1 + k]);
                const float d = rdh1[r] * sp + dh1[r] * sp * (1.0f - 2.0f * h) * rz1;
                sb += d;
                sw = __builtin_fmaf(d, A.ys[n], sw);
            }
            sb = sum_over_rows(sb);
            sw = sum_over_rows(sw);
            if (lq == 0) {  // columns k >= 100 of the last tile hold junk: never read
                A.part[tm * 128 + k] = sb;
                A.part[(RT + tm) * 128 + k] = sw;
            }
        } else {
            const int tm = (job - 7 * RT) & 3, tn = (job - 7 * RT) >> 2, k = 16 * tn + li;
            const f32x4 acc = f4add(lds_tile_mfma<R / 4, kZ2Stride, kH1Ld, false, false, true>(A.Rdz2 + rk * kZ2Stride + 16 * tm + li,
                                                                                              A.h1 + rk * kH1Ld + k),
                                    lds_tile_mfma<R / 4, kZ2Stride, kH1Ld, false, false, true>(A.dz2 + rk * kZ2Stride + 16 * tm + li,
                                                                                              A.Rh1 + rk * kH1Ld + k));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 16 * tm + 4 * lq + r;
                if (m < kH2 && k < kH1) hv[L.w2 + m * kH1Ld + k] += acc[r];
            }
        }
    }
    if (tid >= kTrainThreads - 64 && tid < kTrainThreads - 64 + kH2) {  // R db2, by the last wave
        const int m = tid - (kTrainThreads - 64);
        float dv[R];
#pragma unroll
        for (int n = 0; n < R; ++n) dv[n] = A.Rdz2[n * kZ2Stride + m];
        __builtin_amdgcn_sched_barrier(0);
        float acc = 0.0f;
#pragma unroll
        for (int n = 0; n < R; ++n) acc += dv[n];
        hv[L.b2 + m] += acc;
    }
    __syncthreads();
    // R dW1, R db1: thread t < 50 adds the four floats hv[4 t .. 4 t + 3]; no barrier after it: any other reader of
    // hv[0 .. 199] needs one (the caller's, after the last chunk)
    if (tid < 2 * kH1 / 4) {  // one 16-byte read-modify-write per thread
        const int t4 = tid < kH1 / 4 ? tid : tid - kH1 / 4;
        const float4 *src = reinterpret_cast<const float4 *>(A.part + (tid < kH1 / 4 ? RT * 128 : 0)) + t4;
        float4 a = src[0];
        if (RT > 1) {
            const float4 o = src[128 / 4];
            a = make_float4(a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w);
        }
        float4 *dst = reinterpret_cast<float4 *>(hv) + tid;
        const float4 gv = *dst;
        *dst = make_float4(gv.x + a.x, gv.y + a.y, gv.z + a.z, gv.w + a.w);
    }
}

// ---- pieces of the meta-learning kernels' frame (maml_train_kernel, maml_train_states, maml_train_groups_kernel)
// sample n of a step's support set (W words of T samples) / of its query word
struct MetaSamples {
    const int *__restrict__ support_idx, *__restrict__ query_idx;
    int W, T;
    __device__ __forceinline__ long long support(int step, int n) const { return (long long)support_idx[(long long)step * W + n / T] * T + n % T; }
    __device__ __forceinline__ long long query(int step, int n) const { return (long long)query_idx[step] * T + n; }
};

template <int SC, bool MANY>  // as online_train_kernel: compile-time n_states or 0 = run-time S_rt; one trial by value or trial blockIdx.y
__global__ __launch_bounds__(kTrainThreads) void maml_train_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int W, float meta_lr, int second_order,
    float lr, float beta1, float beta2, float eps, int S_rt, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const mvn_train_trial_t &d = MANY ? many[blockIdx.y] : one;
    const int n_steps = d.n;
    if (n_steps <= 0) return;
    const float *__restrict__ rx_words = d.y;
    const int *__restrict__ labels = d.labels, *__restrict__ support_idx = d.idx, *__restrict__ query_idx = d.query_idx;
    float *__restrict__ adam_m = d.adam_m, *__restrict__ adam_v = d.adam_v, *__restrict__ loss_out = d.loss_out;
    double b1pow = d.b1pow, b2pow = d.b2pow;
    const int S = SC ? SC : S_rt;
    const TrainLayout L = train_layout(S);
    float *th = smem;        // theta
    float *ga = th + L.P4;   // accumulator: support gradient, later H v
    float *gq = ga + L.P4;   // query gradient = the direction v
    float *thp = gq + L.P4;  // where theta waits while theta' (the inner step) sits in `th` for the query pass: dead afterwards ...
    float *arena = thp + L.P4;
    const ChunkArena<kTrainChunk> A(arena);
    const HvArena<kHvRows> HA(thp);  // ... so the Hessian pass's 32-sample images start there (they need the room)
    const int tid = threadIdx.x;

    MVN_CLEAR_LDS_LOAD_PARAMS(kTrainThreads, th);
    __syncthreads();

    const int n_sup = W * T, n_qry = T;
    const float inv_ns = 1.0f / (float)n_sup, inv_nq = 1.0f / (float)n_qry;
    // The two chunk layouts alias each other: before a pass the columns its products rely on being zero are cleared
    // (z2 / dz2 / R a2 / R dz2 columns 50,51; dlogits columns >= S)
    auto clear_pads_grad = [&]() {
        for (int e = tid; e < kTrainChunk * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            A.z2[i] = 0.0f;
            A.dz2[i] = 0.0f;
        }
        for (int e = tid; e < kTrainChunk * kDlStride; e += kTrainThreads)
            if (e % kDlStride >= S) A.dl[e] = 0.0f;
        __syncthreads();
    };
    auto clear_pads_hv = [&]() {
        for (int e = tid; e < kHvRows * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            HA.z2[i] = 0.0f;
            HA.Ra2[i] = 0.0f;
            HA.dz2[i] = 0.0f;
            HA.Rdz2[i] = 0.0f;
        }
        for (int e = tid; e < kHvRows * kDlStride; e += kTrainThreads)
            if (e % kDlStride >= S) {
                HA.dlo[e] = 0.0f;
                HA.Rdo[e] = 0.0f;
            }
        __syncthreads();
    };
    const MetaSamples smp = {support_idx, query_idx, W, T};

    for (int step = 0; step < n_steps; ++step) {
        // (read by everyone at the Adam update)
        auto bias_corrections = [&]() { next_bias_corrections<true>(b1pow, b2pow, lr, beta1, beta2, A.red[kTrainChunk + 1], A.red[kTrainChunk + 2]); };
        // ---- pass 0: g_s = grad L_support(theta);  pass 1: g_q = grad L_query(theta'), theta' = theta - meta_lr g_s.
        // ONE loop over the two passes and the SAME two LDS vectors in both -- the parameters the pass differentiates at in `th`,
        // its gradient in `ga` -- so that the chunk code (the bulk of the kernel) is inlined once per form with every LDS address
        // an immediate: a pointer chosen per pass costs an address add per access (+8 % per chunk, measured), a copy of the chunk
        // code per pass does not fit the instruction cache.  Between the passes theta moves to `thp` and theta' takes its place;
        // afterwards theta comes back and g_q moves to `gq` (6 floats per thread each way).
        clear_pads_grad();
        for (int pass = 0; pass < 2; ++pass) {
            const int n_pass = pass ? n_qry : n_sup;
            const float inv_n = pass ? inv_nq : inv_ns;
            if (pass) {
                for (int e = tid; e < L.P4; e += kTrainThreads) {
                    const float t = th[e];
                    thp[e] = t;
                    th[e] = t - meta_lr * ga[e];  // (ga is rewritten by the query pass's first chunk)
                }
                if (tid == 0) A.red[kTrainChunk] = 0.0f;  // the query loss is the one reported (trainer.py:453)
                __syncthreads();
            }
            for (int c0 = 0; c0 < n_pass; c0 += kTrainChunk) {
                const int nc = n_pass - c0 < kTrainChunk ? n_pass - c0 : kTrainChunk;
                if (tid < kTrainChunk) {
                    const bool valid = tid < nc;
                    const long long s = !valid ? 0 : pass ? smp.query(step, c0 + tid) : smp.support(step, c0 + tid);
                    A.ys[tid] = valid ? rx_words[s] : 0.0f;
                    A.lab[tid] = valid ? labels[s] : 0;
                }
                __syncthreads();
                auto idle = [&]() {
                    if (pass == 0) bias_corrections();
                };
                // three inlined copies: a pass's first chunk, a further full chunk, a further chunk of at most 16 samples
                if (c0 == 0) grad_chunk<kTrainChunk, true>(th, ga, L, A, nc, inv_n, S, idle);
                else if (nc <= 16) grad_chunk<16, false>(th, ga, L, A, nc, inv_n, S);
                else grad_chunk<kTrainChunk, false>(th, ga, L, A, nc, inv_n, S);
            }
        }
        for (int e = tid; e < L.P4; e += kTrainThreads) {
            gq[e] = ga[e];
            ga[e] = 0.0f;  // (the Hessian pass adds to it)
            th[e] = thp[e];
        }
        const float loss_q = A.red[kTrainChunk] * inv_nq;
        const float step_size = A.red[kTrainChunk + 1], inv_sqrt_bc2 = A.red[kTrainChunk + 2];
        __syncthreads();  // the scalars above live in the arena the Hessian pass is about to reuse
        // ---- H_support(theta) g_q -> ga
        if (second_order) {
            clear_pads_hv();
            for (int c0 = 0; c0 < n_sup; c0 += kHvRows) {
                const int nc = n_sup - c0 < kHvRows ? n_sup - c0 : kHvRows;
                if (tid < kHvRows) {
                    const bool valid = tid < nc;
                    const long long s = valid ? smp.support(step, c0 + tid) : 0;
                    HA.ys[tid] = valid ? rx_words[s] : 0.0f;
                    HA.lab[tid] = valid ? labels[s] : 0;
                }
                __syncthreads();
                if (nc <= 16) hv_chunk<16>(th, gq, ga, L, HA, nc, inv_ns, S);
                else hv_chunk<kHvRows>(th, gq, ga, L, HA, nc, inv_ns, S);
            }
            __syncthreads();  // the last chunk's R dW1 / R db1 update of ga[0 .. 199] (threads 0 .. 49)
        }
        // ---- theta <- Adam(theta, g_q - meta_lr H g_q); the moments live in global memory
        for (int e = tid; e < L.Pflat; e += kTrainThreads) {
            const int le = lds_index(e);
            const float gr = second_order ? gq[le] - meta_lr * ga[le] : gq[le];
            float pe = th[le], me = adam_m[e], ve = adam_v[e];
            adam1(pe, me, ve, gr, beta1, beta2, eps, step_size, inv_sqrt_bc2);
            th[le] = pe;
            adam_m[e] = me;
            adam_v[e] = ve;
        }
        if (tid == 0 && loss_out) loss_out[step] = loss_q;
        __syncthreads();
    }
    store_trial_params(th, L, S, d);
}

// ---- 64 and 128 states: maml_train_kernel<64 | 128, false> ---------------------------------------------------------------
// The same step in TWO parameter-sized LDS vectors instead of four (a vector is 34 / 47 KB here):
//   th  theta during the support pass and the Hessian pass, theta' during the query pass
//   ga  the pass's gradient: g_s, then g_q -- which IS the direction v of the Hessian pass, so it stays where it is
// next to one arena that holds the gradient passes' 32-row ChunkArena (dlogits rows of S + 2 floats, as online_train_kernel<64 | 128>)
// or, in its place, the Hessian pass's 16-row HvArena.  What leaves LDS:
//   * theta while theta' sits in `th`: stored to the trial's weight arrays (w_out) before the inner step and reloaded from them
//     after the query pass (one store and one load of the parameters per step; the arrays hold the final weights at the end anyway);
//   * the H v accumulator: with 16-row chunks only, the dealing of tile products to waves is the same in every chunk, so every
//     lane adds to the same elements each time -- they stay in registers (HvRegs, 23 per lane) over the chunk loop and are written
//     once, over the dead arena, for the Adam loop.
// Bytes: 2 x 34 464 + 40 704 + 256 = 109 888 at 64 states, 2 x 47 520 + 52 992 + 256 = 148 288 at 128 (of 163 840).
constexpr int kHvRowsStates = 16;

struct HvRegs {     // a lane's share of H v (hv_chunk_states adds, hv_store writes it out)
    f32x4 w3[2];    // R dW3 tiles wave, wave + 16 of the 4 S / 16 (the second at 128 states only)
    f32x4 w2[2];    // R dW2 tiles wave, wave + 16 of the 28
    float b3[2];    // wave 15: states lane, lane + 64
    float b2;       // wave 15: unit lane
    float4 w1b1;    // threads 0 .. 49: float4 tid of the vector (W1, b1)
};

// hv_chunk for SCC = 64 / 128 states (a compile-time constant, as grad_chunk's SCC) on a 16-sample chunk in a true 16-row arena
// built with dlogits rows of SCC + 2 floats: the softmax phase takes a wave per sample (SCC / 64 states per lane), the products
// over the states run SCC / 4 k-steps, R db3 takes SCC / 64 states per lane, and the SCC / 16 tiles of logits / R o and the
// 4 SCC / 16 tiles of R dW3 are dealt wave by wave.  The sums go to `acc`; no barrier at the end (as hv_chunk).
// (A form of its own, not more branches in hv_chunk: where the sums go, the arena's rows and every phase that knows the state
// count differ; what is shared is lds_tile_mfma and the arithmetic of the header.)
template <int SCC>
__device__ __forceinline__ void hv_chunk_states(const float *p, const float *v, HvRegs &acc, const TrainLayout &L,
                                                const HvArena<kHvRowsStates> &A, int nc, float inv_n) {
    constexpr int R = kHvRowsStates, DLS = SCC + 2, TS = SCC / 16, NK = SCC / 64;
    static_assert(SCC == 64 || SCC == 128, "64 or 128 states");
    static_assert(R == kTrainThreads / 64 && 2 * TS <= kTrainThreads / 64 && TS / 4 <= 2, "a wave per sample; the dealing below");
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // (as hv_chunk: operand addresses are recomputed per call, not kept across the kernel)
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lq = lane >> 4, rk = rows_k_base<R / 4>(lq);
    // ---- layer 1 and its tangent
    for (int e = tid; e < R * kH1; e += kTrainThreads) {
        const int n = e / kH1, k = e % kH1;
        const float h = sigmoid_train(__builtin_fmaf(A.ys[n], p[L.w1 + k], p[L.b1 + k]));
        A.h1[n * kH1Ld + k] = h;
        A.Rh1[n * kH1Ld + k] = h * (1.0f - h) * __builtin_fmaf(A.ys[n], v[L.w1 + k], v[L.b1 + k]);
    }
    __syncthreads();
    // ---- z2 (waves 0 .. 3) and R z2 = W2 R h1 + vW2 h1 + vb2 (waves 4 .. 7): a tile of 16 units each
    if (wave < 8) {
        const bool tangent = wave >= 4;
        const int m = 16 * (wave & 3) + li;
        const float bias = (tangent ? v : p)[L.b2 + (m < kH2 ? m : 0)];
        __builtin_amdgcn_sched_barrier(0);
        if (!tangent) {
            const f32x4 t = lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.h1 + li * kH1Ld + lq, p + L.w2 + m * kH1Ld + lq);
            if (m < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.z2[(4 * lq + r) * kZ2Stride + m] = t[r] + bias;
        } else {
            const f32x4 t = f4add(lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.Rh1 + li * kH1Ld + lq, p + L.w2 + m * kH1Ld + lq),
                                  lds_tile_mfma<kK2Steps, 1, 1, false, false>(A.h1 + li * kH1Ld + lq, v + L.w2 + m * kH1Ld + lq));
            if (m < kH2)
#pragma unroll
                for (int r = 0; r < 4; ++r) A.Ra2[(4 * lq + r) * kZ2Stride + m] = t[r] + bias;
        }
    }
    __syncthreads();
    for (int e = tid; e < R * kH2; e += kTrainThreads) {  // R a2 = R z2 [z2 > 0]
        const int i = (e / kH2) * kZ2Stride + e % kH2;
        A.Ra2[i] = A.z2[i] > 0.0f ? A.Ra2[i] : 0.0f;
    }
    __syncthreads();
    // ---- logits (waves 0 .. TS - 1) and R o = W3 R a2 + vW3 a2 + vb3 (waves TS .. 2 TS - 1)
    if (wave < 2 * TS) {
        const bool tangent = wave >= TS;
        const int s = 16 * (tangent ? wave - TS : wave) + li;  // (< SCC)
        const float bias = (tangent ? v : p)[L.b3 + s];
        __builtin_amdgcn_sched_barrier(0);
        if (!tangent) {
            const f32x4 t = lds_tile_mfma<kK3Steps, 1, 1, true, false>(A.z2 + li * kZ2Stride + lq, p + L.w3 + s * kH2 + lq);
#pragma unroll
            for (int r = 0; r < 4; ++r) A.pr[(4 * lq + r) * DLS + s] = t[r] + bias;
        } else {
            const f32x4 t = f4add(lds_tile_mfma<kK3Steps, 1, 1, false, false>(A.Ra2 + li * kZ2Stride + lq, p + L.w3 + s * kH2 + lq),
                                  lds_tile_mfma<kK3Steps, 1, 1, true, false>(A.z2 + li * kZ2Stride + lq, v + L.w3 + s * kH2 + lq));
#pragma unroll
            for (int r = 0; r < 4; ++r) A.Rdo[(4 * lq + r) * DLS + s] = t[r] + bias;
        }
    }
    __syncthreads();
    // ---- softmax, do and R do = p (R o - <p, R o>) / n: wave n takes sample n, NK states per lane (as grad_chunk's BIG form)
    {
        const int n = wave;
        float x[NK], ro[NK], prob[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            x[k] = A.pr[n * DLS + lane + 64 * k];
            ro[k] = A.Rdo[n * DLS + lane + 64 * k];
        }
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
        const float lg = logf(sum);
        float dot = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            prob[k] = expf((x[k] - mx) - lg);
            dot += prob[k] * ro[k];
        }
        dot = sample_allreduce<false>(dot, 32);
        dot += __shfl_xor(dot, 32);
        const bool live = n < nc;
        const int label = A.lab[n];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int s = lane + 64 * k;
            A.dlo[n * DLS + s] = live ? (prob[k] - (s == label ? 1.0f : 0.0f)) * inv_n : 0.0f;
            A.Rdo[n * DLS + s] = live ? prob[k] * (ro[k] - dot) * inv_n : 0.0f;
        }
    }
    __syncthreads();
    // ---- dz2 (waves 0 .. 3), R dz2 = (W3^T R do + vW3^T do) [z2 > 0] (waves 4 .. 7): SCC / 4 k-steps over the states;
    // R dW3 tiles wave (and wave + 16); R db3 by wave 15
    if (wave < 8) {
        const bool tangent = wave >= 4;
        const int k = 16 * (wave & 3) + li;
        const float *dl_l = A.dlo + li * DLS + lq, *rd_l = A.Rdo + li * DLS + lq;
        const float *w3p = p + L.w3 + lq * kH2 + k, *w3v = v + L.w3 + lq * kH2 + k;
        const int e0 = 4 * lq * kZ2Stride + k;
        float zv[4];  // the mask's z2 values travel with the operands
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = A.z2[e0 + r * kZ2Stride];
        __builtin_amdgcn_sched_barrier(0);
        f32x4 t;
        if (!tangent) t = lds_tile_mfma<SCC / 4, 1, kH2, false, false>(dl_l, w3p);
        else t = f4add(lds_tile_mfma<SCC / 4, 1, kH2, false, false>(rd_l, w3p), lds_tile_mfma<SCC / 4, 1, kH2, false, false>(dl_l, w3v));
        float *dst = A.dz2 + (tangent ? R * kZ2Stride : 0);  // R dz2 follows dz2 (base + offset: the stores stay LDS stores)
        if (k < kH2)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[e0 + r * kZ2Stride] = zv[r] > 0.0f ? t[r] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TS / 4; ++i) {  // R dW3 [S][50] = R do^T a2 + do^T R a2, contraction over the R samples
        const int j = wave + 16 * i, ts = j >> 2, k = 16 * (j & 3) + li;
        acc.w3[i] = f4add(acc.w3[i], f4add(lds_tile_mfma<R / 4, DLS, kZ2Stride, false, true, true>(A.Rdo + rk * DLS + 16 * ts + li,
                                                                                                  A.z2 + rk * kZ2Stride + k),
                                           lds_tile_mfma<R / 4, DLS, kZ2Stride, false, false, true>(A.dlo + rk * DLS + 16 * ts + li,
                                                                                                   A.Ra2 + rk * kZ2Stride + k)));
    }
    if (wave == 15) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            float dv[R];
#pragma unroll
            for (int n = 0; n < R; ++n) dv[n] = A.Rdo[n * DLS + lane + 64 * k];
            __builtin_amdgcn_sched_barrier(0);
            float t = 0.0f;
#pragma unroll
            for (int n = 0; n < R; ++n) t += dv[n];
            acc.b3[k] += t;
        }
    }
    __syncthreads();
    // ---- 7 tiles of R dz1 (waves 0 .. 6); R dW2 = R dz2^T h1 + dz2^T R h1: tiles wave and wave + 16 of the 28; R db2 by wave 15
    if (wave < 7) {
        const int k = 16 * wave + li;
        const float *w2p = p + L.w2 + lq * kH1Ld + k, *w2v = v + L.w2 + lq * kH1Ld + k;
        const f32x4 dh1 = lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.dz2 + li * kZ2Stride + lq, w2p);
        const f32x4 rdh1 = f4add(lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.Rdz2 + li * kZ2Stride + lq, w2p),
                                 lds_tile_mfma<kK3Steps, 1, kH1Ld, false, false>(A.dz2 + li * kZ2Stride + lq, w2v));
        float sb = 0.0f, sw = 0.0f;  // R dz1 stays in registers (as hv_chunk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = 4 * lq + r, e = n * kH1Ld + k;
            const float h = A.h1[e], sp = h * (1.0f - h);
            const float rz1 = __builtin_fmaf(A.ys[n], v[L.w1 + k], v[L.b1 + k]);
            const float d = rdh1[r] * sp + dh1[r] * sp * (1.0f - 2.0f * h) * rz1;
            sb += d;
            sw = __builtin_fmaf(d, A.ys[n], sw);
        }
        sb = sum_over_rows(sb);
        sw = sum_over_rows(sw);
        if (lq == 0) {  // columns k >= 100 of the last tile hold junk: never read
            A.part[k] = sb;
            A.part[128 + k] = sw;
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = wave + 16 * i;
        if (j < 28) {
            const int tm = j & 3, k = 16 * (j >> 2) + li;
            acc.w2[i] = f4add(acc.w2[i], f4add(lds_tile_mfma<R / 4, kZ2Stride, kH1Ld, false, false, true>(A.Rdz2 + rk * kZ2Stride + 16 * tm + li,
                                                                                                         A.h1 + rk * kH1Ld + k),
                                               lds_tile_mfma<R / 4, kZ2Stride, kH1Ld, false, false, true>(A.dz2 + rk * kZ2Stride + 16 * tm + li,
                                                                                                         A.Rh1 + rk * kH1Ld + k)));
        }
    }
    if (wave == 15 && lane < kH2) {
        float dv[R];
#pragma unroll
        for (int n = 0; n < R; ++n) dv[n] = A.Rdz2[n * kZ2Stride + lane];
        __builtin_amdgcn_sched_barrier(0);
        float t = 0.0f;
#pragma unroll
        for (int n = 0; n < R; ++n) t += dv[n];
        acc.b2 += t;
    }
    __syncthreads();
    if (tid < 2 * kH1 / 4) {  // R dW1 (threads 0 .. 24: the sums weighted with the inputs), R db1 (25 .. 49)
        const float4 a = reinterpret_cast<const float4 *>(A.part + (tid < kH1 / 4 ? 128 : 0))[tid < kH1 / 4 ? tid : tid - kH1 / 4];
        acc.w1b1 = make_float4(acc.w1b1.x + a.x, acc.w1b1.y + a.y, acc.w1b1.z + a.z, acc.w1b1.w + a.w);
    }
}

// writes the accumulators to the TrainLayout vector hv[] (every element of the six arrays has exactly one owner: the dealing of
// hv_chunk_states); the caller's barriers before and after
template <int SCC>
__device__ __forceinline__ void hv_store(const HvRegs &acc, float *hv, const TrainLayout &L) {
    constexpr int TS = SCC / 16, NK = SCC / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int i = 0; i < TS / 4; ++i) {
        const int j = wave + 16 * i, ts = j >> 2, k = 16 * (j & 3) + li;
        if (k < kH2)
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[L.w3 + (16 * ts + 4 * lq + r) * kH2 + k] = acc.w3[i][r];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = wave + 16 * i, tm = j & 3, k = 16 * (j >> 2) + li;
        if (j < 28 && k < kH1)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 16 * tm + 4 * lq + r;
                if (m < kH2) hv[L.w2 + m * kH1Ld + k] = acc.w2[i][r];
            }
    }
    if (wave == 15) {
#pragma unroll
        for (int k = 0; k < NK; ++k) hv[L.b3 + lane + 64 * k] = acc.b3[k];
        if (lane < kH2) hv[L.b2 + lane] = acc.b2;
    }
    if (tid < 2 * kH1 / 4) reinterpret_cast<float4 *>(hv)[tid] = acc.w1b1;
}

template <int SC>
__device__ __forceinline__ void maml_train_states(const mvn_train_trial_t &d, int T, int W, float meta_lr, int second_order, float lr,
                                                  float beta1, float beta2, float eps, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n_steps = d.n;
    if (n_steps <= 0) return;
    const float *__restrict__ rx_words = d.y;
    const int *__restrict__ labels = d.labels, *__restrict__ support_idx = d.idx, *__restrict__ query_idx = d.query_idx;
    float *adam_m = d.adam_m, *adam_v = d.adam_v, *loss_out = d.loss_out;
    double b1pow = d.b1pow, b2pow = d.b2pow;
    constexpr int S = SC;
    const TrainLayout L = train_layout(S);
    float *th = smem;        // theta; theta' during the query pass
    float *ga = th + L.P4;   // the pass's gradient; after the query pass the direction v = g_q
    float *arena = ga + L.P4;
    const ChunkArena<kTrainChunk> A(arena, false, SC + 2);
    const HvArena<kHvRowsStates> HA(arena, SC + 2);
    float *hv = arena;  // H v for the Adam loop, written over the Hessian pass's images when they are dead
    const float *const w_wait[6] = {d.w_out[0], d.w_out[1], d.w_out[2], d.w_out[3], d.w_out[4], d.w_out[5]};  // where theta waits
    const int tid = threadIdx.x;

    MVN_CLEAR_LDS_LOAD_PARAMS(kTrainThreads, th);
    __syncthreads();

    const int n_sup = W * T, n_qry = T;
    const float inv_ns = 1.0f / (float)n_sup, inv_nq = 1.0f / (float)n_qry;
    // the two chunk layouts alias each other: before a pass the columns its products rely on being zero are cleared (z2 / dz2 /
    // R a2 / R dz2 columns 50, 51; no product reads a dlogits column >= S here: the contraction over the states is S long)
    auto clear_pads_grad = [&]() {
        for (int e = tid; e < kTrainChunk * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            A.z2[i] = 0.0f;
            A.dz2[i] = 0.0f;
        }
        __syncthreads();
    };
    auto clear_pads_hv = [&]() {
        for (int e = tid; e < kHvRowsStates * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            HA.z2[i] = 0.0f;
            HA.Ra2[i] = 0.0f;
            HA.dz2[i] = 0.0f;
            HA.Rdz2[i] = 0.0f;
        }
        __syncthreads();
    };
    const MetaSamples smp = {support_idx, query_idx, W, T};

    for (int step = 0; step < n_steps; ++step) {
        // (read by everyone at the Adam update)
        auto bias_corrections = [&]() { next_bias_corrections<true>(b1pow, b2pow, lr, beta1, beta2, A.red[kTrainChunk + 1], A.red[kTrainChunk + 2]); };
        // ---- pass 0: g_s = grad L_support(theta);  pass 1: g_q = grad L_query(theta'): one loop, the same two vectors (as above)
        clear_pads_grad();
        for (int pass = 0; pass < 2; ++pass) {
            const int n_pass = pass ? n_qry : n_sup;
            const float inv_n = pass ? inv_nq : inv_ns;
            if (pass) {
                store_params(th, L, S, d.w_out);  // theta waits in the weight arrays
                __syncthreads();
                for (int e = tid; e < L.P4; e += kTrainThreads) th[e] = th[e] - meta_lr * ga[e];  // (ga is rewritten by the first chunk)
                if (tid == 0) A.red[kTrainChunk] = 0.0f;  // the query loss is the one reported (trainer.py:453)
                __syncthreads();
            }
            for (int c0 = 0; c0 < n_pass; c0 += kTrainChunk) {
                const int nc = n_pass - c0 < kTrainChunk ? n_pass - c0 : kTrainChunk;
                if (tid < kTrainChunk) {
                    const bool valid = tid < nc;
                    const long long s = !valid ? 0 : pass ? smp.query(step, c0 + tid) : smp.support(step, c0 + tid);
                    A.ys[tid] = valid ? rx_words[s] : 0.0f;
                    A.lab[tid] = valid ? labels[s] : 0;
                }
                __syncthreads();
                auto idle = [&]() {
                    if (pass == 0) bias_corrections();
                };
                if (c0 == 0) grad_chunk<kTrainChunk, true, kTrainThreads, SC>(th, ga, L, A, nc, inv_n, S, idle);
                else if (nc <= 16) grad_chunk<16, false, kTrainThreads, SC>(th, ga, L, A, nc, inv_n, S);
                else grad_chunk<kTrainChunk, false, kTrainThreads, SC>(th, ga, L, A, nc, inv_n, S);
            }
        }
        const float loss_q = A.red[kTrainChunk] * inv_nq;
        const float step_size = A.red[kTrainChunk + 1], inv_sqrt_bc2 = A.red[kTrainChunk + 2];
        load_params(th, L, S, w_wait);  // theta comes back (theta' is dead: the last chunk ended with a barrier)
        __syncthreads();  // ... and the scalars above live in the arena the Hessian pass is about to reuse
        // ---- H_support(theta) g_q -> hv
        if (second_order) {
            HvRegs acc;
            acc.w3[0] = acc.w3[1] = acc.w2[0] = acc.w2[1] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc.b3[0] = acc.b3[1] = acc.b2 = 0.0f;
            acc.w1b1 = make_float4(0.f, 0.f, 0.f, 0.f);
            clear_pads_hv();
            for (int c0 = 0; c0 < n_sup; c0 += kHvRowsStates) {
                const int nc = n_sup - c0 < kHvRowsStates ? n_sup - c0 : kHvRowsStates;
                if (tid < kHvRowsStates) {
                    const bool valid = tid < nc;
                    const long long s = valid ? smp.support(step, c0 + tid) : 0;
                    HA.ys[tid] = valid ? rx_words[s] : 0.0f;
                    HA.lab[tid] = valid ? labels[s] : 0;
                }
                __syncthreads();
                hv_chunk_states<SC>(th, ga, acc, L, HA, nc, inv_ns);
            }
            __syncthreads();  // the last chunk's images are dead
            hv_store<SC>(acc, hv, L);
            __syncthreads();
        }
        // ---- theta <- Adam(theta, g_q - meta_lr H g_q); the moments live in global memory (kPer elements' loads in flight together)
        constexpr int kPer = 4;
        for (int e0 = tid; e0 < L.Pflat; e0 += kPer * kTrainThreads) {
            float me[kPer], ve[kPer], pe[kPer], ge[kPer];
            int le[kPer];
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int e = e0 + j * kTrainThreads;
                const bool in = e < L.Pflat;
                le[j] = lds_index(in ? e : 0);
                me[j] = in ? adam_m[e] : 0.0f;
                ve[j] = in ? adam_v[e] : 0.0f;
                pe[j] = th[le[j]];
                ge[j] = second_order ? ga[le[j]] - meta_lr * hv[le[j]] : ga[le[j]];
            }
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int e = e0 + j * kTrainThreads;
                if (e < L.Pflat) {
                    adam1(pe[j], me[j], ve[j], ge[j], beta1, beta2, eps, step_size, inv_sqrt_bc2);
                    th[le[j]] = pe[j];
                    adam_m[e] = me[j];
                    adam_v[e] = ve[j];
                }
            }
        }
        if (tid == 0 && loss_out) loss_out[step] = loss_q;
        __syncthreads();
    }
    store_trial_params(th, L, S, d);
}

template <>
__global__ __launch_bounds__(kTrainThreads) void maml_train_kernel<64, false>(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int W, float meta_lr, int second_order,
    float lr, float beta1, float beta2, float eps, int S_rt, int lds_floats) {
    maml_train_states<64>(one, T, W, meta_lr, second_order, lr, beta1, beta2, eps, lds_floats);
}
template <>
__global__ __launch_bounds__(kTrainThreads) void maml_train_kernel<128, false>(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int W, float meta_lr, int second_order,
    float lr, float beta1, float beta2, float eps, int S_rt, int lds_floats) {
    maml_train_states<128>(one, T, W, meta_lr, second_order, lr, beta1, beta2, eps, lds_floats);
}

// ---- R trials at 64 and 128 states: maml_train_states_trials_kernel<64 | 128>, grid (1, R) ----------------------------------
// The same body, the trial being many[blockIdx.y] of a device array (mvn_vnet_maml_train_states_trials_f32).  The step needs no
// workspace and has no barrier between workgroups, so one workgroup IS one trial and the trials of a launch never wait for each
// other: no residency condition applies, R above the CU count runs in ONE launch with gridDim.y = R (a workgroup fills a CU's LDS,
// the dispatcher starts the next trial where one ends).  A trial with n = 0 exits at once and touches nothing.
// What the body asks of the descriptors (include/mvn.h has the contract):
//   * theta waits in d.w_out between the two gradient passes of every step (store_params before the inner step, load_params
//     after the query pass), so w_out holds intermediate values while the launch runs and must belong to this trial alone;
//   * d.w_in is read once, by the load_params before the first step, and never again: it may be the trial's own w_out or
//     w_out2 (the saved row, written only by store_trial_params at the end) or a row all trials share read-only;
//   * `status` is never written (nothing here can give up); loss_out may be NULL.
// The descriptor is a reference into global memory instead of a kernel argument; blockIdx.y is uniform, so its pointers and
// n / b1pow / b2pow arrive by scalar loads as the by-value form's do from the kernel-argument segment.
template <int SC>
__global__ __launch_bounds__(kTrainThreads) void maml_train_states_trials_kernel(
    const mvn_train_trial_t *__restrict__ many, int T, int W, float meta_lr, int second_order, float lr, float beta1, float beta2,
    float eps, int lds_floats) {
    static_assert(SC == 64 || SC == 128, "64 or 128 states (up to 32: maml_train_kernel<SC, true>)");
    maml_train_states<SC>(many[blockIdx.y], T, W, meta_lr, second_order, lr, beta1, beta2, eps, lds_floats);
}

// floats of one parameter vector in LDS (train_layout's P4)
constexpr int train_p4(int S) { return (2 * kH1 + kH2 * kH1Ld + kH2 + S * kH2 + S + 3) & ~3; }
constexpr size_t maml_train_lds_floats(int S) {
    // + 64: operand rows read past the last image stay inside the allocation
    if (S > 32) {  // theta and one gradient, then the gradient passes' arena or, in its place, the Hessian pass's 16-row arena
        const int grad = ChunkArena<kTrainChunk>::floats(S + 2), hess = HvArena<kHvRowsStates>::floats(S + 2);
        return (size_t)2 * train_p4(S) + (grad > hess ? grad : hess) + 64;
    }
    // theta, two accumulators, then theta' + the gradient passes' arena or, in their place, the Hessian pass's arena
    const int grad = train_p4(S) + ChunkArena<kTrainChunk>::kFloats, hess = HvArena<kHvRows>::kFloats;
    return (size_t)3 * train_p4(S) + (grad > hess ? grad : hess) + 64;
}
constexpr size_t kCuLdsBytes = 163840;
static_assert(maml_train_lds_floats(64) * sizeof(float) <= kCuLdsBytes && maml_train_lds_floats(128) * sizeof(float) <= kCuLdsBytes,
              "maml_train_kernel<64 | 128, false>: two vectors and an arena in one CU's LDS");
static_assert(train_p4(128) <= HvArena<kHvRowsStates>::floats(128 + 2) && train_p4(64) <= HvArena<kHvRowsStates>::floats(64 + 2),
              "H v is written over the Hessian pass's arena");
