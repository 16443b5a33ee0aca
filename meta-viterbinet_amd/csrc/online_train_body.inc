// online_train_body.inc -- the body of online_train_kernel and of online_train_words_kernel (online_train.inc), included once
// into each as a TEXT: shared as a function it changes the code of every online_train_kernel instantiation
// (tools/kernel_isa_diff.py, profiles/train_words_isa_identity.txt).  The includer defines MVN_TRAIN_WORDS:
//   0: one word, y / labels [T] -- token for token the body online_train_kernel had before the word axis;
//   1: the word axis (joint training, the inner loop of Trainer.train(), trainer.py:470-479): y [n_words, ld_y], labels
//      [n_words, ld_lab], iteration `it` trains on row word_of_iter[it] (the descriptor's query_idx), T counts the labelled
//      positions of a word; ld_y / ld_lab are kernel arguments.
// In scope: SC, MANY, NT (template parameters or constants) and the kernel arguments one, many, T, M, lr, beta1, beta2, eps, S_rt,
// lds_floats.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const mvn_train_trial_t &d = MANY ? many[blockIdx.y] : one;
    const int n_iter = d.n;
    if (n_iter <= 0) return;
    const float *__restrict__ y = d.y;
    const int *__restrict__ labels = d.labels, *__restrict__ batch_idx = d.idx;
    float *__restrict__ adam_m = d.adam_m, *__restrict__ adam_v = d.adam_v, *__restrict__ loss_out = d.loss_out;
    double b1pow = d.b1pow, b2pow = d.b2pow;
    const int S = SC ? SC : S_rt;
    const TrainLayout L = train_layout(S);
    // SC = 64 / 128 (round 5): parameters + gradient are 69 / 95 KB and the arena (dlogits rows of SC + 2 floats) 36 / 44 KB: one
    // 1024-thread workgroup with the moments in global memory, like the 512-thread form
    constexpr int SCC = SC > 32 ? SC : 0;  // grad_chunk's compile-time state count above 32
    constexpr bool kMomentsInLds = NT == kTrainThreads && SC <= 32;
    static_assert(SC <= 32 || NT == kTrainThreads, "64 / 128 / 256 states: 1024-thread workgroups");
    // SC = 256: parameters 73.6 KB, arena 62.3 KB -- the gradient vector goes without dW3 (22.4 KB instead of 73.6), which lives in
    // the 16 accumulator registers dw3 of every thread across a pass (grad_chunk) and meets Adam there (apply_dw3_from_regs)
    constexpr bool kW3Regs = SC > kGradW3InLdsStates;
    static_assert(!kW3Regs || !MANY, "256 states: one trial");
    f32x4 dw3[kW3Regs ? 4 : 1];
    float *p = smem;       // parameters
    float *g = p + L.P4;   // gradient accumulators
    float *am = g + L.P4;  // Adam exp_avg    } (NT = 1024 up to 32 states; otherwise they stay in global memory)
    float *av = am + L.P4; // Adam exp_avg_sq }
    const ChunkArena<kTrainChunk> A(kMomentsInLds ? av + L.P4 : g + (kW3Regs ? L.P4 - SC * kH2 : L.P4), NT != kTrainThreads,
                                    SCC ? SCC + 2 : kDlStride);
    const int tid = threadIdx.x;

    MVN_CLEAR_LDS_LOAD_PARAMS(NT, p);
    if (kMomentsInLds) moments_to_lds<NT>(am, av, adam_m, adam_v, L.Pflat, tid);
    __syncthreads();

    const int n_total = batch_idx ? M : T;  // samples per iteration
    const float inv_n = 1.0f / (float)n_total;
    // threads < 32 prefetch in two stages so that no load waits on another inside an iteration: the sample index of the
    // chunk after next (s_next2), then sample and label of the next chunk through the index fetched one chunk earlier
    float y_next = 0.0f;
    int lab_next = 0, s_next2 = 0;
#if MVN_TRAIN_WORDS
    // The word of a chunk is the same for its 32 samples, and the chunk whose index is being fetched may belong to a later iteration,
    // hence to another word, than the chunk being computed: the word travels with the sample index.  It does so in the SAME
    // register: the 32 prefetching lanes are the lower half of the first wave, the upper half of every one of their registers is
    // idle, so lanes 32..63 fetch word_of_iter[it_] into their s_next2 in the stage that fetches the index (two independent loads,
    // the pipeline keeps its depth) and fetch_sample reads it from lane 32 -- when it waits for the index anyway.  No further vector
    // register is held across the chunk (one more spills in the 128-state form), and no load waits on another.
    // word_at() reads word_of_iter[k] for k < n_iter only, and fetch_index reads batch_idx only behind it_ < n_iter: the two
    // prefetches that run past the last iteration read neither array, s_next2 = -1 there and fetch_sample loads nothing.
    const int *__restrict__ word_of_iter = d.query_idx;
    auto word_at = [&](int it_) { return it_ < n_iter ? word_of_iter[it_] : 0; };
    constexpr int kWordLane = kTrainChunk;  // lanes kTrainChunk .. 63 all hold the word; this one is read
#endif
    auto advance = [&](int &it_, int &c0_) {
        c0_ += kTrainChunk;
        if (c0_ >= n_total) {
            c0_ = 0;
            ++it_;
        }
    };
    auto fetch_index = [&](int it_, int c0_) {  // -1: padding row / past the last iteration
#if MVN_TRAIN_WORDS
        if (tid >= kTrainChunk) {
            s_next2 = word_at(it_);
            return;
        }
#endif
        const bool valid = it_ < n_iter && c0_ + tid < n_total;
        s_next2 = valid ? (batch_idx ? batch_idx[(long long)it_ * M + c0_ + tid] : c0_ + tid) : -1;
    };
    auto fetch_sample = [&]() {
#if MVN_TRAIN_WORDS
        const int w_ = __builtin_amdgcn_readlane(s_next2, kWordLane);
        const bool take = tid < kTrainChunk && s_next2 >= 0;  // (the upper lanes hold the word, not a sample)
        y_next = take ? y[(long long)w_ * ld_y + s_next2] : 0.0f;
        lab_next = take ? labels[(long long)w_ * ld_lab + s_next2] : 0;
#else
        y_next = s_next2 >= 0 ? y[s_next2] : 0.0f;
        lab_next = s_next2 >= 0 ? labels[s_next2] : 0;
#endif
    };
    int it_pf = 0, c_pf = 0;  // position of the chunk whose index is fetched next
#if MVN_TRAIN_WORDS
    if (tid < 64) {  // (the first wave: its lower half prefetches the samples, its upper half their word)
#else
    if (tid < kTrainChunk && n_iter > 0) {
#endif
        fetch_index(it_pf, c_pf);
        fetch_sample();
        advance(it_pf, c_pf);
        fetch_index(it_pf, c_pf);
    }
    // the fetched samples go to the arena -- the first chunk's here, every other one's at the end of the chunk before it
    auto stage_chunk = [&]() {
#if MVN_TRAIN_WORDS
        if (tid < 64) {
            if (tid < kTrainChunk) {
                A.ys[tid] = y_next;
                A.lab[tid] = lab_next;
            }
#else
        if (tid < kTrainChunk) {
            A.ys[tid] = y_next;
            A.lab[tid] = lab_next;
#endif
            fetch_sample();  // the chunk after, through the index requested one chunk ago
            advance(it_pf, c_pf);
            fetch_index(it_pf, c_pf);
        }
    };
    stage_chunk();
    __syncthreads();
    for (int it = 0; it < n_iter; ++it) {
#ifdef MVN_DIAG_TRAIN
        if (tid == 0) g_diag_on = it == 100;
        TRAIN_STAMP(8);
#endif
        if (tid == NT - 1) A.red[kTrainChunk] = 0.0f;  // running loss of this iteration
        // Adam's bias corrections in double like torch's Python side, by one lane of the last wave while it idles in
        // the first chunk's first matrix product; everyone reads them after the barriers in between
        auto bias_corrections = [&]() { next_bias_corrections<false>(b1pow, b2pow, lr, beta1, beta2, A.red[kTrainChunk + 1], A.red[kTrainChunk + 2]); };
        // three inlined copies of the chunk code (it is the bulk of the kernel; the instruction cache holds 64 KB): the pass's
        // first chunk, a further full chunk, a further chunk of at most 16 samples
        for (int c0 = 0; c0 < n_total; c0 += kTrainChunk) {
            const int nc = n_total - c0 < kTrainChunk ? n_total - c0 : kTrainChunk;
            if (c0 == 0) grad_chunk<kTrainChunk, true, NT, SCC>(p, g, L, A, nc, inv_n, S, bias_corrections, stage_chunk, kW3Regs ? dw3 : nullptr);
            else if (nc <= 16) grad_chunk<16, false, NT, SCC>(p, g, L, A, nc, inv_n, S, NoHook(), stage_chunk, kW3Regs ? dw3 : nullptr);
            else grad_chunk<kTrainChunk, false, NT, SCC>(p, g, L, A, nc, inv_n, S, NoHook(), stage_chunk, kW3Regs ? dw3 : nullptr);
        }
        const float step_size = A.red[kTrainChunk + 1], inv_sqrt_bc2 = A.red[kTrainChunk + 2];
        if constexpr (MVN_ABL(7)) {
        } else if constexpr (kMomentsInLds) {  // float4 tid and float4 tid + 1024 of the vectors (P4 / 4 <= 2048 for every S <= 32), all eight reads in one round trip
            const int e4b = tid + kTrainThreads < L.P4 / 4 ? tid + kTrainThreads : tid;
            float4 *const P = reinterpret_cast<float4 *>(p), *const M = reinterpret_cast<float4 *>(am);
            float4 *const V = reinterpret_cast<float4 *>(av);
            const float4 *const G = reinterpret_cast<const float4 *>(g);
            float4 pa = P[tid], ma = M[tid], va = V[tid], pb = P[e4b], mb = M[e4b], vb = V[e4b];
            const float4 ga = G[tid], gb = G[e4b];
            __builtin_amdgcn_sched_barrier(0);
            adam4(pa, ma, va, ga, beta1, beta2, eps, step_size, inv_sqrt_bc2);
            M[tid] = ma;
            V[tid] = va;
            P[tid] = pa;  // (g[] is left as it is: the next iteration's first chunk overwrites it)
            if (e4b != tid) {
                adam4(pb, mb, vb, gb, beta1, beta2, eps, step_size, inv_sqrt_bc2);
                M[e4b] = mb;
                V[e4b] = vb;
                P[e4b] = pb;
            }
        } else if constexpr (kW3Regs) {  // as below for everything but W3: element i < w3_flat of the flat vectors, then b3
            // 5 506 elements, six per thread, all their loads in flight at once.  An element past the end takes element 0's place
            // in the loads (no branch around a load: the compiler otherwise waits for each on its own) and stores nothing.
            constexpr int kW3 = SC * kH2, kW3Flat = 2 * kH1 + kH2 * kH1 + kH2, kRest = kW3Flat + SC, kPer = (kRest + NT - 1) / NT;
            float me[kPer], ve[kPer], pe[kPer], ge[kPer];
            int le[kPer];
            unsigned ee[kPer];  // (unsigned: a 32-bit offset from the uniform base pointer)
            int t_ = tid;  // opaque: the offsets are recomputed per iteration, not kept (and spilled) across the chunks
            asm volatile("" : "+v"(t_));
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int i = t_ + j * NT < kRest ? t_ + j * NT : 0;
                ee[j] = (unsigned)(i < kW3Flat ? i : i + kW3);
                le[j] = lds_index((int)ee[j]);
                me[j] = adam_m[ee[j]];
                ve[j] = adam_v[ee[j]];
                pe[j] = p[le[j]];
                ge[j] = g[i < kW3Flat ? le[j] : le[j] - kW3];  // (db3 follows db2 in g[])
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kPer; ++j)
                if (t_ + j * NT < kRest) {
                    adam1(pe[j], me[j], ve[j], ge[j], beta1, beta2, eps, step_size, inv_sqrt_bc2);
                    p[le[j]] = pe[j];
                    adam_m[ee[j]] = me[j];
                    adam_v[ee[j]] = ve[j];
                }
            apply_dw3_from_regs(p, L, dw3, adam_m, adam_v, beta1, beta2, eps, step_size, inv_sqrt_bc2);
        } else {  // moments in global memory, element e of the flat (torch-order) vectors: coalesced; the same adam1 per element
            constexpr int kPer = 4;  // elements whose loads are in flight together
            for (int e0 = tid; e0 < L.Pflat; e0 += kPer * NT) {
                float me[kPer], ve[kPer], pe[kPer], ge[kPer];
                int le[kPer];
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const int e = e0 + j * NT;
                    const bool in = e < L.Pflat;
                    le[j] = lds_index(in ? e : 0);
                    me[j] = in ? adam_m[e] : 0.0f;
                    ve[j] = in ? adam_v[e] : 0.0f;
                    pe[j] = p[le[j]];
                    ge[j] = g[le[j]];
                }
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const int e = e0 + j * NT;
                    if (e < L.Pflat) {
                        adam1(pe[j], me[j], ve[j], ge[j], beta1, beta2, eps, step_size, inv_sqrt_bc2);
                        p[le[j]] = pe[j];
                        adam_m[e] = me[j];
                        adam_v[e] = ve[j];
                    }
                }
            }
        }
        if (tid == 0 && loss_out) loss_out[it] = A.red[kTrainChunk] * inv_n;
        TRAIN_STAMP_WAVE(7);
        __syncthreads();
#ifdef MVN_DIAG_TRAIN
        TRAIN_STAMP(9);
#endif
    }
#ifdef MVN_DIAG_TRAIN
    if (tid == 0 && loss_out && n_iter >= 102 + 2 * 152)  // 152 stamps of iteration 100 as 304 dwords from loss_out[102]
        for (int k = 0; k < 152; ++k) reinterpret_cast<unsigned long long *>(loss_out + 102)[k] = g_diag_stamps[k];
#endif

    store_trial_params<NT>(p, L, S, d);
    if (kMomentsInLds) moments_from_lds<NT>(am, av, adam_m, adam_v, L.Pflat, tid);
