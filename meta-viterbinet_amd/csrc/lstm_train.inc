// lstm_train.inc -- training of the windowed two-layer LSTM detector (lstm.inc) in ONE launch: n_iter x {forward 'train' on one
// word, CrossEntropyLoss(mean), backward through time, optimizer step}, the loop of LSTMTrainer.online_training
// (trainers/LSTM/lstm_trainer.py:42-53: M sampled positions per iteration), MetaLSTMTrainer.online_training
// (trainers/META_LSTM/meta_lstm_trainer.py:48-60: the whole word) and, with a word index per iteration, the inner loop of
// Trainer.train() (trainer.py:470-479).  Included by mvn_hip.hip after train_groups.inc and lstm.inc.
//
// The batch is one word, so an iteration is a serial chain of 1024 x 256 mat-vecs; the 3.2 MB of weights do not fit one CU.
// lstm_train_kernel runs on kLtGroups = 64 workgroups of 256 threads, one per CU.  Workgroup g OWNS hidden units 4g .. 4g+3 of
// both layers, i.e. gate rows n = 256 gate + 4g + uu (local row r = 4 gate + uu) of every matrix, and keeps in LDS
//   * those 16 rows of W_hh0, W_ih1, W_hh1 (forward products, and the rows whose gradient and optimizer step it computes),
//   * columns 4g .. 4g+3 of the same three matrices (backward: dh[k] = sum_n W[n][k] dgate[n] for ITS OWN k, so the backward
//     product is an all-gather of dgates like the forward one is of h, never a sum across workgroups),
//   * i, f, g, o, c of its 8 units for all T steps (overwritten by the four gate gradients on the way back).
// Per time step the workgroups exchange h (forward; layer 1 of step s-1 runs beside layer 0 of step s, so ONE exchange serves
// both) or dgates (backward, the same skew): 2 (T + 1) exchanges per iteration, each one groups_barrier of train_groups.inc --
// write-through (sc1) stores, every storing wave's s_waitcnt, one lane's arrival and bounded sc1 poll, sc1 loads.  h of all
// steps stays in the workspace ([layer][t][256]): the weight gradients dW[n][k] = sum_t dgate_t[n] in_t[k] of the owned rows are
// formed after the sweep, thread k holding the 48 sums of column k, t ascending.  The optimizer step (adam1: Adam, RMSprop or
// SGD by the beta1 tag) then runs on the owner's slice only, moments in global memory; one more device-wide barrier, and every
// workgroup re-reads its column copies and the fc layer.
// Every sum has a fixed order (16-lane xor trees, t ascending) and every parameter has one owner, so a call is bit-reproducible,
// and since all state passes through global memory after every iteration and the bias corrections are a function of the absolute
// step number (pow_int below), n iterations in one call equal n1 + n2 in two.
// A wait that is abandoned (spin limit, train_groups.inc) is sticky: every workgroup leaves its loops, writes NaN over the
// parameters it owns and sets *status = 1.
// lstm_maml_kernel is the same body run twice per step (support pass, query pass): first-order online meta-learning, see
// LstmMetaArgs below.
// lstm_train_trials_kernel / lstm_maml_trials_kernel run the same body for up to 8 independent trials in one launch, 64 workgroups
// and one workspace region each (LstmTrialsArgs below).
constexpr int kLtGroups = 64, kLtThreads = 256, kLtU = kLstmH / kLtGroups, kLtR = 4 * kLtU;
constexpr int kLstmTrainMaxT = 256;       // LDS: 40 T floats of saved activations beside 96 KB of weights
constexpr int kLstmTrainMaxIter = 8192;   // iterations per launch (the arrival counter is 32 bits wide)
static_assert(kLtU == 4 && kLtR == 16 && kLtThreads == kLstmH, "thread k <-> column k; 16 lanes per owned row");
// parameters() order offsets into exp_avg / exp_avg_sq
constexpr size_t kLtOff[10] = {0, 4096, 266240, 267264, 268288, 530432, 792576, 793600, 794624, 795136};
constexpr size_t kLstmParams = 795138;

struct LstmTrainArgs {
    const float *y;
    long long y_ld;
    const int *bits;
    long long bits_ld;
    const int *word_of_iter, *idx;
    int M, n_iter;
    float *w[10];
    float *m, *v;
    long long step0;
    float lr, beta1, beta2, eps;
    float *loss_out;
    float *ws;
    unsigned ws_bytes;  // SlotIO addresses the workspace with 32-bit byte offsets: 540 KB at kLstmTrainMaxT, far inside
    int *status;
    int T;
    unsigned spin_limit;
};

// workspace, in floats: GroupSync, h of both layers for all steps, the dgates exchange [layer][step parity][1024]
__host__ __device__ constexpr size_t lt_ws_hist() { return sizeof(GroupSync) / sizeof(float); }
__host__ __device__ constexpr size_t lt_ws_dg(int T) { return lt_ws_hist() + (size_t)2 * T * kLstmH; }
__host__ __device__ constexpr size_t lt_ws_floats(int T) { return lt_ws_dg(T) + 4 * kLstmGates; }
// LDS, in floats
struct LtLds {
    int wrow, wcol, wih0, bias, fcw, hbuf, dgbuf, part, yw, lab, idx, dl, nll, cnt, saved, total;
    __host__ __device__ explicit LtLds(int T) {
        const int Tp = (T + 3) & ~3;
        int o = 0;
        auto take = [&](int n) { const int at = o; o += (n + 3) & ~3; return at; };
        wrow = take(3 * kLtR * kLstmH);
        wcol = take(3 * kLtU * kLstmGates);
        wih0 = take(kLtR * kLstmIn);
        bias = take(4 * kLtR);
        fcw = take(2 * kLstmH + 4);
        hbuf = take(2 * kLstmH);
        dgbuf = take(2 * kLstmGates);
        part = take(3 * kLtR);
        yw = take(Tp + 4);
        lab = take(Tp);
        idx = take(Tp);
        dl = take(2 * Tp);
        nll = take(Tp);
        cnt = take(Tp);
        saved = take(2 * kLtU * 5 * Tp);
        total = o;
    }
};
inline size_t lstm_train_lds_bytes(int T) { return (size_t)LtLds(T).total * sizeof(float); }

// beta^n in double by squaring: a function of the absolute step number alone (what makes split calls bit-identical)
__device__ __forceinline__ double pow_int(double b, long long n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

__device__ __forceinline__ float lt_reduce16(float v) {  // sum over the 16 lanes of a row, fixed tree
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// Online meta-learning (first-order MAML, Trainer.meta_train_loop with MAML=False, trainer.py:425-453) on the same sweeps: META runs
// the loop body TWICE per step.  The support pass (word support_of_step[k]) ends in theta' = fl(theta - meta_lr g_s) instead of the
// optimizer step: theta' replaces the LDS working copies and goes, for the three big matrices and the fc layer, to a fast-weight
// image behind the training workspace, from which every workgroup re-reads its column copies and the fc layer after the pass's
// closing barrier; a.w[] and the moments are not touched.  The query pass (word word_of_iter[k]) runs at theta', its loss is
// loss_out[k], and its gradient -- the first-order meta-gradient -- drives adam1 on THETA, which the owner reads back from a.w[].
// One support word, first order only: the second-order term needs a tangent copy of the weights that LDS has no room for.
struct LstmMetaArgs : LstmTrainArgs {
    const int *support_of_step;
    float meta_lr;
};
// the fast-weight image, in floats from its base: W_hh0, W_ih1, W_hh1, fc weight, fc bias
constexpr size_t kLtFastHh0 = 0, kLtFastIh1 = (size_t)kLstmGates * kLstmH, kLtFastHh1 = 2 * kLtFastIh1, kLtFastFc = 3 * kLtFastIh1;
constexpr size_t kLtFastFcb = kLtFastFc + 2 * kLstmH, kLtFastFloats = kLtFastFcb + 4;
__host__ __device__ constexpr size_t lt_maml_ws_floats(int T) { return lt_ws_floats(T) + kLtFastFloats; }

template <bool META, class Args>
__device__ __forceinline__ void lstm_train_body(const Args a, const int g) {  // (by value: a reference costs lstm_train_kernel three VGPRs)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T = a.T, Tp = (T + 3) & ~3, M = a.M;
    const LtLds L(T);
    float *wrow = smem + L.wrow, *wcol = smem + L.wcol, *wih0 = smem + L.wih0, *bias = smem + L.bias, *fcw = smem + L.fcw;
    float *hbuf = smem + L.hbuf, *dgbuf = smem + L.dgbuf, *part = smem + L.part, *yw = smem + L.yw, *dl = smem + L.dl;
    float *nll = smem + L.nll, *cnt = smem + L.cnt, *saved = smem + L.saved;
    int *lab = reinterpret_cast<int *>(smem + L.lab), *idxs = reinterpret_cast<int *>(smem + L.idx);
    const int tid = threadIdx.x;  // g: this workgroup's group number within its trial
    GroupSync *gs = reinterpret_cast<GroupSync *>(a.ws);
    const SlotIO io(a.ws, a.ws_bytes);  // same_xcd stays false: write-through stores, sc1 loads
    const SlotIO mhh0(a.w[1], kLstmGates * kLstmH * 4), mih1(a.w[4], kLstmGates * kLstmH * 4), mhh1(a.w[5], kLstmGates * kLstmH * 4);
    const SlotIO fcio(a.w[8], 2 * kLstmH * 4), fcbio(a.w[9], 8);
    const SlotIO fio(META ? a.ws + lt_ws_floats(T) : a.ws, (unsigned)(kLtFastFloats * 4));  // META only: the fast-weight image
    const size_t H0 = lt_ws_hist(), H1 = H0 + (size_t)T * kLstmH, DG = lt_ws_dg(T);
    auto row_of = [&](int r) { return 256 * (r >> 2) + kLtU * g + (r & 3); };  // local row -> gate row of the matrices
    auto sv = [&](int l, int uu, int q, int t) -> float & { return saved[((l * kLtU + uu) * 5 + q) * Tp + t]; };

    // this workgroup's rows (plain loads: nobody has written them in this launch yet) and small tensors
    for (int e = tid; e < kLtR * kLstmH; e += kLtThreads) {
        const size_t at = (size_t)row_of(e / kLstmH) * kLstmH + e % kLstmH;
        wrow[e] = a.w[1][at];
        wrow[kLtR * kLstmH + e] = a.w[4][at];
        wrow[2 * kLtR * kLstmH + e] = a.w[5][at];
    }
    if (tid < kLtR * kLstmIn) wih0[tid] = a.w[0][row_of(tid >> 2) * kLstmIn + (tid & 3)];
    if (tid < kLtR) {
        const int n = row_of(tid);
        bias[tid] = a.w[2][n];
        bias[kLtR + tid] = a.w[3][n];
        bias[2 * kLtR + tid] = a.w[6][n];
        bias[3 * kLtR + tid] = a.w[7][n];
    }
    // column copies wcol[m][kk][n]: m = 0 W_hh1, 1 W_ih1, 2 W_hh0; and the fc layer
    auto read_from = [&](const SlotIO &shh1, const SlotIO &sih1, const SlotIO &shh0, const SlotIO &sfc, const SlotIO &sfcb, size_t ohh1,
                         size_t oih1, size_t ohh0, size_t ofc, size_t ofcb) {
        for (int n = tid; n < kLstmGates; n += kLtThreads) {
            const size_t at = (size_t)n * kLstmH + kLtU * g;
            const float4 v[3] = {shh1.load4(ohh1 + at), sih1.load4(oih1 + at), shh0.load4(ohh0 + at)};
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float *dst = wcol + (m * kLtU) * kLstmGates + n;
                dst[0] = v[m].x;
                dst[kLstmGates] = v[m].y;
                dst[2 * kLstmGates] = v[m].z;
                dst[3 * kLstmGates] = v[m].w;
            }
        }
        if (tid < 2 * kLstmH / 4) reinterpret_cast<float4 *>(fcw)[tid] = sfc.load4(ofc + 4 * (size_t)tid);
        if (tid < 2) fcw[2 * kLstmH + tid] = sfcb.load1(ofcb + tid);
    };
    auto read_shared = [&]() { read_from(mhh1, mih1, mhh0, fcio, fcbio, 0, 0, 0, 0, 0); };
    auto read_fast = [&]() { read_from(fio, fio, fio, fio, fio, kLtFastHh1, kLtFastIh1, kLtFastHh0, kLtFastFc, kLtFastFcb); };
    read_shared();
    if (tid < 3) yw[tid] = kLstmPad;
    __syncthreads();

    unsigned epoch = 0;
    bool good = true;
    const int sub = tid & 15, grp = tid >> 4;
    const int n_pass = META ? 2 * a.n_iter : a.n_iter;  // META: support pass, query pass of step k = it / 2
    for (int it = 0; it < n_pass && good; ++it) {
        const bool query = !META || (it & 1);
        const int k = META ? it >> 1 : it;
        long long word;
        if constexpr (META) word = query ? a.word_of_iter[k] : a.support_of_step[k];
        else word = a.word_of_iter ? a.word_of_iter[it] : 0;
        if (tid < T) {
            yw[3 + tid] = a.y[word * a.y_ld + tid];
            lab[tid] = a.bits[word * a.bits_ld + tid];
        }
        if (tid < M) idxs[tid] = a.idx[(long long)it * M + tid];
        // ---- forward: step s runs layer 0 at t = s and layer 1 at t = s - 1
        for (int s = 0; s <= T && good; ++s) {
            hbuf[tid] = s >= 1 ? io.load1(H0 + (size_t)(s - 1) * kLstmH + tid) : 0.0f;
            hbuf[kLstmH + tid] = s >= 2 ? io.load1(H1 + (size_t)(s - 2) * kLstmH + tid) : 0.0f;
            __syncthreads();
            {
                float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
                const float4 *w0 = reinterpret_cast<const float4 *>(wrow + (0 * kLtR + grp) * kLstmH);
                const float4 *w1 = reinterpret_cast<const float4 *>(wrow + (1 * kLtR + grp) * kLstmH);
                const float4 *w2 = reinterpret_cast<const float4 *>(wrow + (2 * kLtR + grp) * kLstmH);
                const float4 *x0 = reinterpret_cast<const float4 *>(hbuf), *x1 = reinterpret_cast<const float4 *>(hbuf + kLstmH);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = sub + 16 * j;
                    const float4 h0v = x0[q], h1v = x1[q], a0 = w0[q], a1 = w1[q], a2 = w2[q];
                    p0 = fmaf(a0.x, h0v.x, p0); p0 = fmaf(a0.y, h0v.y, p0); p0 = fmaf(a0.z, h0v.z, p0); p0 = fmaf(a0.w, h0v.w, p0);
                    p1 = fmaf(a1.x, h0v.x, p1); p1 = fmaf(a1.y, h0v.y, p1); p1 = fmaf(a1.z, h0v.z, p1); p1 = fmaf(a1.w, h0v.w, p1);
                    p2 = fmaf(a2.x, h1v.x, p2); p2 = fmaf(a2.y, h1v.y, p2); p2 = fmaf(a2.z, h1v.z, p2); p2 = fmaf(a2.w, h1v.w, p2);
                }
                p0 = lt_reduce16(p0);
                p1 = lt_reduce16(p1);
                p2 = lt_reduce16(p2);
                if (sub == 0) {
                    part[grp] = p0;
                    part[kLtR + grp] = p1 + p2;
                }
            }
            __syncthreads();
            if (tid < 2 * kLtU) {
                const int l = tid >> 2, uu = tid & 3, t = l ? s - 1 : s;
                if (t >= 0 && t < T) {
                    float z[4];
#pragma unroll
                    for (int gt = 0; gt < 4; ++gt) {
                        const int r = 4 * gt + uu;
                        float acc = bias[(2 * l) * kLtR + r] + bias[(2 * l + 1) * kLtR + r];
                        if (l == 0) {
#pragma unroll
                            for (int j = 0; j < kLstmIn; ++j) acc = fmaf(wih0[r * kLstmIn + j], yw[t + j], acc);
                        }
                        z[gt] = acc + part[l * kLtR + r];
                    }
                    const float ig = sigmoid_from_neg(0.0f - z[0]), fg = sigmoid_from_neg(0.0f - z[1]);
                    const float gg = lstm_tanh(z[2]), og = sigmoid_from_neg(0.0f - z[3]);
                    const float cp = t > 0 ? sv(l, uu, 4, t - 1) : 0.0f;
                    const float cn = fg * cp + ig * gg;
                    sv(l, uu, 0, t) = ig;
                    sv(l, uu, 1, t) = fg;
                    sv(l, uu, 2, t) = gg;
                    sv(l, uu, 3, t) = og;
                    sv(l, uu, 4, t) = cn;
                    io.store1((l ? H1 : H0) + (size_t)t * kLstmH + kLtU * g + uu, og * lstm_tanh(cn));
                }
            }
            good = groups_barrier(gs, kLtGroups, epoch, a.spin_limit) && good;
        }
        if (!good) break;
        // ---- logits, loss and dlogits: every workgroup computes all of them, identically (thread t = time t)
        if (tid < T) {
            float l0 = fcw[2 * kLstmH], l1 = fcw[2 * kLstmH + 1];
            const float4 *f0 = reinterpret_cast<const float4 *>(fcw), *f1 = reinterpret_cast<const float4 *>(fcw + kLstmH);
#pragma unroll 8
            for (int q = 0; q < kLstmH / 4; ++q) {
                const float4 hv = io.load4(H1 + (size_t)tid * kLstmH + 4 * q), u0 = f0[q], u1 = f1[q];
                l0 = fmaf(u0.x, hv.x, l0); l0 = fmaf(u0.y, hv.y, l0); l0 = fmaf(u0.z, hv.z, l0); l0 = fmaf(u0.w, hv.w, l0);
                l1 = fmaf(u1.x, hv.x, l1); l1 = fmaf(u1.y, hv.y, l1); l1 = fmaf(u1.z, hv.z, l1); l1 = fmaf(u1.w, hv.w, l1);
            }
            const float mx = fmaxf(l0, l1), e0 = expf(l0 - mx), e1 = expf(l1 - mx), se = e0 + e1;
            const int lb = lab[tid];
            float c = 1.0f;
            if (M > 0) {
                int n = 0;
                for (int j = 0; j < M; ++j) n += idxs[j] == tid;
                c = (float)n;
            }
            const float scale = c / (float)(M > 0 ? M : T);
            nll[tid] = (mx + logf(se)) - (lb ? l1 : l0);
            cnt[tid] = scale;
            dl[2 * tid] = (e0 / se - (lb ? 0.0f : 1.0f)) * scale;
            dl[2 * tid + 1] = (e1 / se - (lb ? 1.0f : 0.0f)) * scale;
        }
        __syncthreads();
        if (g == 0 && tid < 64 && a.loss_out && query) {  // sum_t scale_t nll_t: lane-strided partial sums, then a fixed tree
            float sum = 0.0f;
            for (int t = tid; t < T; t += 64) sum += cnt[t] * nll[t];
            for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
            if (tid == 0) a.loss_out[k] = sum;
        }
        // ---- backward through time: step s runs layer 1 at t = s and layer 0 at t = s + 1
        float carry = 0.0f;  // threads < 8: dc(t + 1) f(t + 1) of this thread's (layer, unit)
        for (int s = T - 1; s >= -1 && good; --s) {
            {
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                reinterpret_cast<float4 *>(dgbuf)[tid] = s + 1 < T ? io.load4(DG + (size_t)(2 + ((s + 1) & 1)) * kLstmGates + 4 * tid) : zero;
                reinterpret_cast<float4 *>(dgbuf + kLstmGates)[tid] = s + 2 < T ? io.load4(DG + (size_t)((s + 2) & 1) * kLstmGates + 4 * tid) : zero;
            }
            __syncthreads();
            if (grp < 3 * kLtU) {  // part[4 m + kk] = sum_n wcol[m][kk][n] dgate[n]
                const float4 *wc = reinterpret_cast<const float4 *>(wcol + grp * kLstmGates);
                const float4 *d = reinterpret_cast<const float4 *>(dgbuf + (grp < 2 * kLtU ? 0 : kLstmGates));
                float p = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float4 wv = wc[sub + 16 * j], dv = d[sub + 16 * j];
                    p = fmaf(wv.x, dv.x, p); p = fmaf(wv.y, dv.y, p); p = fmaf(wv.z, dv.z, p); p = fmaf(wv.w, dv.w, p);
                }
                p = lt_reduce16(p);
                if (sub == 0) part[grp] = p;
            }
            __syncthreads();
            if (tid < 2 * kLtU) {
                const int l = tid >> 2, uu = tid & 3, t = l ? s : s + 1;
                if (t >= 0 && t < T) {
                    float dh;
                    if (l) {
                        const int k = kLtU * g + uu;
                        dh = part[uu] + fmaf(fcw[kLstmH + k], dl[2 * t + 1], fcw[k] * dl[2 * t]);
                    } else {
                        dh = part[kLtU + uu] + part[2 * kLtU + uu];
                    }
                    const float ig = sv(l, uu, 0, t), fg = sv(l, uu, 1, t), gg = sv(l, uu, 2, t), og = sv(l, uu, 3, t);
                    const float cn = sv(l, uu, 4, t), cp = t > 0 ? sv(l, uu, 4, t - 1) : 0.0f;
                    const float tc = lstm_tanh(cn);
                    const float dc = dh * og * (1.0f - tc * tc) + carry;
                    carry = dc * fg;
                    const float zi = dc * gg * ig * (1.0f - ig), zf = dc * cp * fg * (1.0f - fg);
                    const float zg = dc * ig * (1.0f - gg * gg), zo = dh * tc * og * (1.0f - og);
                    sv(l, uu, 0, t) = zi;
                    sv(l, uu, 1, t) = zf;
                    sv(l, uu, 2, t) = zg;
                    sv(l, uu, 3, t) = zo;
                    if (s >= 0) {
                        const size_t at = DG + (size_t)(2 * l + (t & 1)) * kLstmGates + kLtU * g + uu;
                        io.store1(at, zi);
                        io.store1(at + 256, zf);
                        io.store1(at + 512, zg);
                        io.store1(at + 768, zo);
                    }
                }
            }
            if (s >= 0) good = groups_barrier(gs, kLtGroups, epoch, a.spin_limit) && good;
            else __syncthreads();
        }
        if (!good) break;
        // ---- weight gradients of the owned rows (thread k = column k, t ascending) and the optimizer step
        const long long step = a.step0 + k + 1;
        const float step_size = train_step_size(a.lr, a.beta1, a.beta1 >= 0.0f ? pow_int((double)a.beta1, step) : 0.0);
        const float inv_sqrt_bc2 = a.beta1 >= 0.0f ? (float)(1.0 / sqrt(1.0 - pow_int((double)a.beta2, step))) : 1.0f;
        // one parameter (global, element e of the flat moments); returns via *pp.  META: the support pass takes the inner step
        // p - meta_lr g (one rounding each, like torch) on the working copy; the query pass steps theta, which theta() reads back
        auto update = [&](float *pp, size_t e, float gr, auto theta) {
            if constexpr (META) {
                if (!query) {
                    const float fast = __fsub_rn(*pp, __fmul_rn(a.meta_lr, gr));
                    *pp = fast;
                    return fast;
                }
            }
            float p = META ? theta() : *pp, m = a.m[e], v = a.v[e];
            adam1(p, m, v, gr, a.beta1, a.beta2, a.eps, step_size, inv_sqrt_bc2);
            if (a.beta1 >= 0.0f) a.m[e] = m;
            if (a.beta1 > -1.5f) a.v[e] = v;
            *pp = p;
            return p;
        };
        // a shared parameter's new value: write-through to its tensor, or (META, support pass) to the fast-weight image
        auto put = [&](const SlotIO &real, size_t fast_at, size_t e, float v) {
            if (META && !query) fio.store1(fast_at + e, v);
            else real.store1(e, v);
        };
        {
            float acc0[kLtR], acc1[kLtR], acc2[kLtR], fc0 = 0.0f, fc1 = 0.0f;
#pragma unroll
            for (int r = 0; r < kLtR; ++r) acc0[r] = acc1[r] = acc2[r] = 0.0f;
            float h0p = 0.0f, h1p = 0.0f;
#pragma unroll 2
            for (int t = 0; t < T; ++t) {
                const float h0c = io.load1(H0 + (size_t)t * kLstmH + tid), h1c = io.load1(H1 + (size_t)t * kLstmH + tid);
#pragma unroll
                for (int r = 0; r < kLtR; ++r) {
                    const float d0 = sv(0, r & 3, r >> 2, t), d1 = sv(1, r & 3, r >> 2, t);
                    acc0[r] = fmaf(d0, h0p, acc0[r]);
                    acc1[r] = fmaf(d1, h0c, acc1[r]);
                    acc2[r] = fmaf(d1, h1p, acc2[r]);
                }
                fc0 = fmaf(dl[2 * t], h1c, fc0);
                fc1 = fmaf(dl[2 * t + 1], h1c, fc1);
                h0p = h0c;
                h1p = h1c;
            }
#pragma unroll
            for (int r = 0; r < kLtR; ++r) {
                const size_t e = (size_t)row_of(r) * kLstmH + tid;
                float *w0 = wrow + (0 * kLtR + r) * kLstmH + tid, *w1 = w0 + kLtR * kLstmH, *w2 = w1 + kLtR * kLstmH;
                put(mhh0, kLtFastHh0, e, update(w0, kLtOff[1] + e, acc0[r], [&] { return mhh0.load1(e); }));
                put(mih1, kLtFastIh1, e, update(w1, kLtOff[4] + e, acc1[r], [&] { return mih1.load1(e); }));
                put(mhh1, kLtFastHh1, e, update(w2, kLtOff[5] + e, acc2[r], [&] { return mhh1.load1(e); }));
            }
            if ((tid >> 2) == g) {  // the fc columns of the owned units
                put(fcio, kLtFastFc, tid, update(fcw + tid, kLtOff[8] + tid, fc0, [&] { return fcio.load1(tid); }));
                put(fcio, kLtFastFc, kLstmH + tid, update(fcw + kLstmH + tid, kLtOff[8] + kLstmH + tid, fc1, [&] { return fcio.load1(kLstmH + tid); }));
            }
        }
        if (tid < kLtR * kLstmIn) {  // W_ih0[row][j]
            const int r = tid >> 2, j = tid & 3;
            float acc = 0.0f;
            for (int t = 0; t < T; ++t) acc = fmaf(sv(0, r & 3, r >> 2, t), yw[t + j], acc);
            const size_t e = (size_t)row_of(r) * kLstmIn + j;
            const float p = update(wih0 + tid, kLtOff[0] + e, acc, [&] { return a.w[0][e]; });  // (owner-only: its own plain store)
            if (query) a.w[0][e] = p;
        } else if (tid < kLtR * kLstmIn + 2 * kLtR) {  // b_ih and b_hh of a layer share one gradient
            const int l = (tid - kLtR * kLstmIn) >> 4, r = tid & 15;
            float acc = 0.0f;
            for (int t = 0; t < T; ++t) acc += sv(l, r & 3, r >> 2, t);
            const int n = row_of(r);
            float *bi = l ? a.w[6] : a.w[2], *bh = l ? a.w[7] : a.w[3];
            const float pi = update(bias + (2 * l) * kLtR + r, (l ? kLtOff[6] : kLtOff[2]) + n, acc, [&] { return bi[n]; });
            const float ph = update(bias + (2 * l + 1) * kLtR + r, (l ? kLtOff[7] : kLtOff[3]) + n, acc, [&] { return bh[n]; });
            if (query) {
                bi[n] = pi;
                bh[n] = ph;
            }
        } else if (g == 0 && tid < kLtR * kLstmIn + 2 * kLtR + 2) {  // fc bias
            const int c = tid - (kLtR * kLstmIn + 2 * kLtR);
            float acc = 0.0f;
            for (int t = 0; t < T; ++t) acc += dl[2 * t + c];
            put(fcbio, kLtFastFcb, c, update(fcw + 2 * kLstmH + c, kLtOff[9] + c, acc, [&] { return fcbio.load1(c); }));
        }
        good = groups_barrier(gs, kLtGroups, epoch, a.spin_limit) && good;
        if (good && it + 1 < n_pass) {
            if (META && !query) read_fast();
            else read_shared();
            __syncthreads();
        }
    }
    // after the last barrier nobody waits any more: the sticky flag tells every workgroup whether any wait was abandoned
    if (good && !trial_failed(gs)) return;
    const float nan = __int_as_float(0x7fc00000);
    for (int e = tid; e < kLtR * kLstmH; e += kLtThreads) {
        const size_t at = (size_t)row_of(e / kLstmH) * kLstmH + e % kLstmH;
        a.w[1][at] = nan;
        a.w[4][at] = nan;
        a.w[5][at] = nan;
    }
    if (tid < kLtR * kLstmIn) a.w[0][row_of(tid >> 2) * kLstmIn + (tid & 3)] = nan;
    if (tid < kLtR) {
        const int n = row_of(tid);
        a.w[2][n] = a.w[3][n] = a.w[6][n] = a.w[7][n] = nan;
    }
    if (tid < kLtU) a.w[8][kLtU * g + tid] = a.w[8][kLstmH + kLtU * g + tid] = nan;
    if (g == 0 && tid < 2) a.w[9][tid] = nan;
    if (tid == 0 && a.status) *a.status = 1;
}

__global__ __launch_bounds__(kLtThreads) void lstm_train_kernel(const LstmTrainArgs a) { lstm_train_body<false>(a, blockIdx.x); }
__global__ __launch_bounds__(kLtThreads) void lstm_maml_kernel(const LstmMetaArgs a) { lstm_train_body<true>(a, blockIdx.x); }

// ---- the trial axis: n <= P independent trials in ONE launch of 64 n workgroups.  Workgroup b serves trial slot b / 64 as group
// b % 64 and runs the body above on that trial's arguments: its own words, weights, moments, loss vector, status word and
// workspace region (GroupSync, h history, dgates exchange, fast-weight image), so trials share nothing, finish independently, and
// a trial whose wait is abandoned marks itself alone.  With the dispatcher's round-robin over the XCDs (observed, not promised)
// every trial has 8 workgroups on every XCD; nothing depends on it.  The training LDS is above 96 KB for every T, so a CU holds
// one workgroup, and the launcher keeps 64 n <= CUs: the whole grid is resident, and every spin stays bounded all the same.
constexpr int kLtMaxTrials = 8;
struct LstmTrialSlot {
    const float *y;
    const int *bits;
    const int *word_of_iter, *idx;  // meta-learning: the query words, the support words
    float *params, *m, *v;          // the ten tensors flat in parameters() order (kLtOff), the moments
    float *loss_out;
    float *ws;
    int *status;
    long long step0;
    int n_iter, pad;
};
struct LstmTrialsArgs {
    LstmTrialSlot slot[kLtMaxTrials];
    long long y_ld, bits_ld;
    int M, T;
    float lr, beta1, beta2, eps, meta_lr;
    unsigned spin_limit;
};

template <bool META>
__device__ __forceinline__ void lstm_trials_body(const LstmTrialsArgs &t) {
    const LstmTrialSlot &s = t.slot[blockIdx.x / kLtGroups];
    std::conditional_t<META, LstmMetaArgs, LstmTrainArgs> a;
    a.y = s.y;
    a.y_ld = t.y_ld;
    a.bits = s.bits;
    a.bits_ld = t.bits_ld;
    a.word_of_iter = s.word_of_iter;
    a.idx = META ? nullptr : s.idx;
    a.M = META ? 0 : t.M;
    a.n_iter = s.n_iter;
#pragma unroll
    for (int i = 0; i < 10; ++i) a.w[i] = s.params + kLtOff[i];
    a.m = s.m;
    a.v = s.v;
    a.step0 = s.step0;
    a.lr = t.lr;
    a.beta1 = t.beta1;
    a.beta2 = t.beta2;
    a.eps = t.eps;
    a.loss_out = s.loss_out;
    a.ws = s.ws;
    a.ws_bytes = (unsigned)(lt_ws_floats(t.T) * sizeof(float));
    a.status = s.status;
    a.T = t.T;
    a.spin_limit = t.spin_limit;
    if constexpr (META) {
        a.support_of_step = s.idx;
        a.meta_lr = t.meta_lr;
    }
    lstm_train_body<META>(a, (int)(blockIdx.x % kLtGroups));
}
__global__ __launch_bounds__(kLtThreads) void lstm_train_trials_kernel(const LstmTrialsArgs t) { lstm_trials_body<false>(t); }
__global__ __launch_bounds__(kLtThreads) void lstm_maml_trials_kernel(const LstmTrialsArgs t) { lstm_trials_body<true>(t); }

// n_iter iterations in launches of at most kLstmTrainMaxIter; the arrival counter is zeroed in front of each
int launch_lstm_train(LstmTrainArgs a, hipStream_t st) {
    if (current_device_cus() < kLtGroups) return MVN_E_DEVICE;  // one workgroup per CU, all resident at once
    const size_t lds = lstm_train_lds_bytes(a.T);
    if (int e = ensure_dynamic_lds((const void *)lstm_train_kernel, lstm_train_lds_bytes(kLstmTrainMaxT))) return e;
    a.spin_limit = group_spin_limit();
    const int total = a.n_iter;
    for (int done = 0; done < total; done += kLstmTrainMaxIter) {
        const int n = std::min(kLstmTrainMaxIter, total - done);
        hipError_t e = hipMemsetAsync(a.ws, 0, sizeof(GroupSync), st);
        if (e != hipSuccess) return (int)e;
        LstmTrainArgs b = a;
        b.n_iter = n;
        b.step0 = a.step0 + done;
        if (a.word_of_iter) b.word_of_iter = a.word_of_iter + done;
        if (a.idx) b.idx = a.idx + (long long)done * a.M;
        if (a.loss_out) b.loss_out = a.loss_out + done;
        hipLaunchKernelGGL(lstm_train_kernel, dim3(kLtGroups), dim3(kLtThreads), lds, st, b);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return MVN_OK;
}

// n_steps meta-learning steps in launches of at most kLstmTrainMaxIter / 2 (two passes of the loop body per step)
int launch_lstm_maml(LstmMetaArgs a, hipStream_t st) {
    if (current_device_cus() < kLtGroups) return MVN_E_DEVICE;
    const size_t lds = lstm_train_lds_bytes(a.T);
    if (int e = ensure_dynamic_lds((const void *)lstm_maml_kernel, lstm_train_lds_bytes(kLstmTrainMaxT))) return e;
    a.spin_limit = group_spin_limit();
    const int total = a.n_iter, per = kLstmTrainMaxIter / 2;
    for (int done = 0; done < total; done += per) {
        hipError_t e = hipMemsetAsync(a.ws, 0, sizeof(GroupSync), st);
        if (e != hipSuccess) return (int)e;
        LstmMetaArgs b = a;
        b.n_iter = std::min(per, total - done);
        b.step0 = a.step0 + done;
        b.word_of_iter = a.word_of_iter + done;
        b.support_of_step = a.support_of_step + done;
        if (a.loss_out) b.loss_out = a.loss_out + done;
        hipLaunchKernelGGL(lstm_maml_kernel, dim3(kLtGroups), dim3(kLtThreads), lds, st, b);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return MVN_OK;
}

// P, the trials of one launch: min(8, CUs / 64), MVN_LSTM_TRIALS_PER_LAUNCH=1..8 pins it lower (tests, A/B runs); 0 below 64 CUs
int lstm_trials_per_launch() {
    const int fit = std::min(kLtMaxTrials, current_device_cus() / kLtGroups);
    const char e = sw(SW_LSTM_TRIALS_PER_LAUNCH);
    return e >= '1' && e <= '8' ? std::min(fit, e - '0') : fit;
}

// The trials of a call with n_iter > 0, in trial order, P at a time on the stream; a trial with more iterations than a launch
// holds (kLstmTrainMaxIter passes of the loop body) continues in the next launches of its batch, advanced like launch_lstm_train
// advances it.  The arrival counters of a launch's trials are zeroed in front of it.
template <bool META>
int launch_lstm_trials(const LstmTrialSlot *trials, int R, LstmTrialsArgs shared, hipStream_t st) {
    const int P = lstm_trials_per_launch();
    if (P < 1) return MVN_E_DEVICE;
    const auto kernel = META ? lstm_maml_trials_kernel : lstm_train_trials_kernel;
    const size_t lds = lstm_train_lds_bytes(shared.T);
    if (int e = ensure_dynamic_lds((const void *)kernel, lstm_train_lds_bytes(kLstmTrainMaxT))) return e;
    shared.spin_limit = group_spin_limit();
    const int per = META ? kLstmTrainMaxIter / 2 : kLstmTrainMaxIter;
    int r = 0;
    while (r < R) {
        LstmTrialSlot batch[kLtMaxTrials];
        int nb = 0;
        for (; r < R && nb < P; ++r)
            if (trials[r].n_iter > 0) batch[nb++] = trials[r];
        for (;;) {
            int n = 0;
            for (int b = 0; b < nb; ++b) {
                LstmTrialSlot &left = batch[b];
                if (left.n_iter <= 0) continue;
                LstmTrialSlot &s = shared.slot[n++];
                s = left;
                s.n_iter = std::min(per, left.n_iter);
                hipError_t e = hipMemsetAsync(s.ws, 0, sizeof(GroupSync), st);
                if (e != hipSuccess) return (int)e;
                left.n_iter -= s.n_iter;
                left.step0 += s.n_iter;
                if (left.word_of_iter) left.word_of_iter += s.n_iter;
                if (left.idx) left.idx += META ? (long long)s.n_iter : (long long)s.n_iter * shared.M;
                if (left.loss_out) left.loss_out += s.n_iter;
            }
            if (!n) break;
            for (int b = n; b < kLtMaxTrials; ++b) shared.slot[b] = LstmTrialSlot{};
            hipLaunchKernelGGL(kernel, dim3(kLtGroups * n), dim3(kLtThreads), lds, st, shared);
            if (int rc = (int)hipGetLastError()) return rc;
        }
    }
    return MVN_OK;
}
