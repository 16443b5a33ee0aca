// byword_step_states_va.inc -- the by-word block step (byword_step.inc) for the CLASSICAL Viterbi detector at 4, 8, 32, 64 and 128
// states (included by mvn_hip.hip after byword_list_states.inc): mvn_va_byword_step_states_f32 (the running decision),
// mvn_va_byword_step_states_path_f32 (the traced-back path) and mvn_va_byword_step_states_list_f32 (its list decode).
//
// The frame is byword_step_states.inc's -- one workgroup of kStatesWaves waves per word, an LDS image [t][S], one barrier, one wave
// from there on -- and everything after the barrier IS that family's code: states_sweep_word, states_path_word, byword_list_tail and
// byword_codec are called as they stand.  What differs is phase 1 and the LDS plan:
//   phase 1  no MLP: the branch cost of stage t out of state s is va_cost(y[t], prior[s]) (va_detector.py:64-68; mvn_hip.hip's one
//            definition, the 16-state VA kernels' constant), priors = row r % Bp of state_priors [Bp, S].  The shared wave-0 functions
//            read the image as LOGITS and form the cost as -logit, so the image holds -cost: negation is exact and keeps a NaN a NaN,
//            hence m + -(-cost) == m + cost bit for bit in the sweep, in the beta recursion (delta) and in the candidates' metrics M.
//            512 threads, 512 % S == 0: a thread keeps ONE state (one prior in a register) and strides over the symbols, so a wave's
//            stores are consecutive floats and its loads of y are 64 / S (or one) broadcast addresses.  All eight waves take part because
//            the image is T S values of three operations each -- 17 408 at T = 136, S = 128 -- which one wave would spend 272 rounds on.
//   LDS      StepShared<NS> (the list: ListFields<StepShared<NS>>) is all the static part: there is no W3 image, so the words may be
//            longer than ViterbiNet's at 64 and 128 states: states_va_max_symbols<S>() / states_va_list_max_symbols<S>().
// The lone wave always runs min2_torch_dev (torch.min: NaN when either candidate is), so there is no guard launch as at 16 states.
// A pilot step detects nothing and is the running kernel's (state_priors and rx may then be NULL: they are not touched).

// the longest word of the running and the path step at S states: what the LDS holds next to the larger (NS = 8) static part, in whole
// bytes of eight symbols, and no more than the step's own limit (StepShared's images)
template <int S>
constexpr int states_va_max_symbols() {
    constexpr size_t fixed = (sizeof(StepShared<8>) + 15) / 16 * 16;
    static_assert(fixed < kStatesLdsBytes, "the static part alone fills the LDS");
    constexpr size_t t = (kStatesLdsBytes - fixed) / (4 * (size_t)S) / 8 * 8;
    return t < (size_t)kCoopMaxT ? (int)t : kCoopMaxT;
}

template <int NS>
using StatesVaListShared = ListFields<StepShared<NS>>;

// the longest word of the list step at S states (states_list_symbol_bytes: the image, the alpha half-image, the survivors), no more than
// kListMaxT (the ranking takes one byte per lane)
template <int S>
constexpr int states_va_list_max_symbols() {
    constexpr size_t fixed = (sizeof(StatesVaListShared<8>) + 15) / 16 * 16;
    static_assert(fixed < kStatesLdsBytes, "the static part alone fills the LDS");
    constexpr size_t t = (kStatesLdsBytes - fixed) / states_list_symbol_bytes<S>() / 8 * 8;
    return t < (size_t)kListMaxT ? (int)t : kListMaxT;
}

// Phase 1 by the whole workgroup: image[t][s] = -va_cost(y[t], prior[s]), t < T.  Thread i keeps state i % S and takes the symbols
// i / S, i / S + 512 / S, ...
template <int S>
__device__ __forceinline__ void states_va_costs(float *image, const float *__restrict__ y, const float *__restrict__ prior, int T) {
    constexpr int kThreads = 64 * kStatesWaves, TS = kThreads / S;  // symbols per round of the workgroup
    static_assert(kThreads % S == 0, "a thread keeps one state");
    const int s = threadIdx.x & (S - 1);
    const float p = prior[s];
#pragma unroll 4
    for (int t = threadIdx.x / S; t < T; t += TS) image[t * S + s] = -va_cost(y[t], p);
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_step_states_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    using C = StatesCfg<S>;
    __shared__ StepShared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // -cost[t][S], t < T (a data step's)
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = T >> 3, k = n - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    if (!pilot) states_va_costs<S>(states_logit, rx + r * rx_ld, priors + (r % Bp) * S, T);  // ---- phase 1
    __syncthreads();
    if (wave != 0) return;
    if (!pilot) {
        // ---- phase 2: wave 0 sweeps the word
        float *decb = dec ? dec + r * dec_ld : nullptr;
        unsigned char *dbits = sh.dbits;
        states_sweep_word<S>(states_logit, T, lane, [&](int t, float mydec) {
            if (decb) decb[t] = mydec;
            dbits[t] = (unsigned char)mydec;
        });
    }
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, C::MEM>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_path_step_states_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym) {
    using C = StatesCfg<S>;
    __shared__ StepShared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // -cost[t][S], t < T; then the survivors, a row per stage
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    states_va_costs<S>(states_logit, rx + r * rx_ld, priors + (r % Bp) * S, T);  // ---- phase 1
    __syncthreads();
    if (wave != 0) return;
    // ---- phase 2: wave 0 sweeps the word, walks its survivors back and carries on with the codec
    states_path_word<S>(states_logit, nullptr, nullptr, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_codec<NS, false, C::MEM>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_list_step_states_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, float *__restrict__ delta_out, int64_t delta_ld, int *__restrict__ choice_out, int T, int nsym,
    int m, int ncand) {
    __shared__ StatesVaListShared<NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // -cost[t][S], then alpha[t][S / 2], then the survivors; t < T
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = (T >> 3) - nsym;

    gf_load(&sh.gf);
    {
        const float *txb = tx ? tx + r * tx_ld : nullptr;  // (no transmitted word: a decoder, nothing is counted)
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x)
            sh.txrow[p] = txb ? (unsigned char)pack_byte(txb + 8 * p) : (unsigned char)0;
    }
    states_va_costs<S>(states_logit, rx + r * rx_ld, priors + (r % Bp) * S, T);  // ---- phase 1
    __syncthreads();
    if (wave != 0) return;
    // ---- phase 2: wave 0 sweeps the word, walks its survivors back, list-decodes and carries on with the codec
    float *alpha = states_logit + T * S;
    unsigned *surv = reinterpret_cast<unsigned *>(alpha + T * (S / 2));
    states_path_word<S, true>(states_logit, alpha, surv, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    byword_list_tail<NS, S>(sh, states_logit, alpha, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out},
                            {delta_out, delta_ld, choice_out, m, ncand}, T, nsym);
}
