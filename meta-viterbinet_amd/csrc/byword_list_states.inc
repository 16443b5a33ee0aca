// byword_list_states.inc -- the by-word block step with the RELIABILITY-ORDERED LIST DECODE (byword_step.inc: byword_list_step_kernel)
// for the ViterbiNet detector at 4, 8, 32, 64 and 128 states (included by mvn_hip.hip after byword_step_states.inc):
// mvn_vnet_byword_step_states_list_f32.
//
// The definition is the 16-state list step's with 16 replaced by S (include/mvn.h); the frame is byword_path_step_states_kernel's:
// eight waves, phase 1 through mlp_tile into the LDS image logit[t][S], one barrier, one wave from there on.  That wave runs
// states_path_word<S, true> (byword_step_states.inc) and byword_list_tail<NS, S> (byword_step.inc): this file holds the kernel, its LDS
// plan and the longest word.  What differs from the path step and from the 16-state list step:
//   sweep   states_path_word's LIST form: the image KEEPS its logits (the candidates' metrics read them again), the stage's
//           survivor ballot goes to an array of its own (one dword per stage up to 32 states, two above), and the metric before stage
//           t goes to an alpha HALF-image [t][S / 2]: states s and s + S / 2 have the same two predecessors, so alpha_t[s] ==
//           alpha_t[s + S / 2] at every t.
//   walk    torch.argmin of the final metrics and the walk back, the survivors fetched from that array: dec, bit for bit the path step's.
//   beta    beta_T = 0, beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | S / 2]), cost = -logit.  A lane holds the
//           PAIR of states h and h + S / 2 (h = lane mod S / 2), so gamma_t[h] = min(beta_t[h], beta_t[h + S / 2]) is an in-lane min and
//           the recursion is beta_{t-1}[p] = cost[t-1][p] + gamma_t[p >> 1]: one cross-lane fetch for each of the lane's two states.
//           Rounded addition is monotone, so min(alpha + beta_a, alpha + beta_b) == alpha + min(beta_a, beta_b) bit for bit on
//           finite values: ab_t[h] = alpha_t[h] + gamma_t[h] overwrites the alpha half-image and is all delta needs.
//   delta   delta_t = min_{h odd} ab_t[h] - min_{h even} ab_t[h] (S / 2 is even: h and h + S / 2 have one parity), a lane per symbol.
//   rank, candidates, choice   as at 16 states: byword_list_tail's one copy, on this kernel's LDS.
//   metric  M(c) = sum_t cost[t][state_t(c)] in ascending t, state_t = sum_{i < log2 S} 2^i b[t + i]: the bit field of the candidate's
//           bytes, reversed.
//   codec   byword_codec<NS, true, log2 S> on the chosen codeword.
// Dynamic LDS: 4 S + 2 S + (4 or 8) bytes per symbol; states_list_max_symbols<S>() is the ONE place that says how long a word may be.
// Non-finite costs: dec keeps the path step's rules, every rank, position, state and candidate index stays in range, delta and
// choice are not specified.
template <int S, int NS>
using StatesListShared = ListFields<StatesStepShared<S, NS>>;  // the list's fields (byword_step.inc) on this family's step

// bytes of dynamic LDS per symbol: the logits, the alpha half-image, the survivors
template <int S>
constexpr size_t states_list_symbol_bytes() {
    return 4 * (size_t)S + 2 * (size_t)S + (S <= 32 ? 4 : 8);
}

// the longest word the list step serves at S states: what the LDS holds next to the larger (NS = 8) static part, in whole bytes of
// eight symbols, and no more than kListMaxT (the ranking takes one byte per lane)
template <int S>
constexpr int states_list_max_symbols() {
    constexpr size_t fixed = (sizeof(StatesListShared<S, 8>) + 15) / 16 * 16;
    static_assert(fixed < kStatesLdsBytes, "the static part alone fills the LDS");
    constexpr size_t t = (kStatesLdsBytes - fixed) / states_list_symbol_bytes<S>() / 8 * 8;
    return t < (size_t)kListMaxT ? (int)t : kListMaxT;
}

template <int S, int NS>
__global__ __launch_bounds__(64 * kStatesWaves) void byword_list_step_states_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, float *__restrict__ delta_out, int64_t delta_ld,
    int *__restrict__ choice_out, int T, int nsym, int m, int ncand) {
    using C = StatesCfg<S>;
    __shared__ StatesListShared<S, NS> sh;
    extern __shared__ __attribute__((aligned(16))) float states_logit[];  // logit[t][S], then alpha[t][S / 2], then the survivors; t < T
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
    MVN_STATES_PHASE1()  // ---- phase 1: the word's tiles, round-robin over the waves (byword_step_states.inc)
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
