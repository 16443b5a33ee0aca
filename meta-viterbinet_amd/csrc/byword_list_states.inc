// byword_list_states.inc -- the by-word block step with the RELIABILITY-ORDERED LIST DECODE (byword_step.inc: byword_list_step_kernel)
// for the ViterbiNet detector at 4, 8, 32, 64 and 128 states (included by mvn_hip.hip after byword_step_states.inc):
// mvn_vnet_byword_step_states_list_f32.
//
// The definition is the 16-state list step's with 16 replaced by S (include/mvn.h); the frame is byword_path_step_states_kernel's:
// eight waves, phase 1 through mlp_tile into the LDS image logit[t][S], one barrier, one wave from there on.  What that wave does:
//   sweep   states_path_word's recurrence, but the image KEEPS its logits (the candidates' metrics read them again): the stage's
//           survivor ballot goes to an array of its own (one dword per stage up to 32 states, two above), and the metric before stage
//           t goes to an alpha HALF-image [t][S / 2]: states s and s + S / 2 have the same two predecessors, so alpha_t[s] ==
//           alpha_t[s + S / 2] at every t.
//   walk    torch.argmin of the final metrics and the walk back, as in states_path_word: dec, bit for bit the path step's.
//   beta    beta_T = 0, beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | S / 2]), cost = -logit.  A lane holds the
//           PAIR of states h and h + S / 2 (h = lane mod S / 2), so gamma_t[h] = min(beta_t[h], beta_t[h + S / 2]) is an in-lane min and
//           the recursion is beta_{t-1}[p] = cost[t-1][p] + gamma_t[p >> 1]: one cross-lane fetch for each of the lane's two states.
//           Rounded addition is monotone, so min(alpha + beta_a, alpha + beta_b) == alpha + min(beta_a, beta_b) bit for bit on
//           finite values: ab_t[h] = alpha_t[h] + gamma_t[h] overwrites the alpha half-image and is all delta needs.
//   delta   delta_t = min_{h odd} ab_t[h] - min_{h even} ab_t[h] (S / 2 is even: h and h + S / 2 have one parity), a lane per symbol.
//   rank, candidates, choice   byword_list_tail's lines (byword_step.inc), on this kernel's LDS.
//   metric  M(c) = sum_t cost[t][state_t(c)] in ascending t, state_t = sum_{i < log2 S} 2^i b[t + i]: the bit field of the candidate's
//           bytes, reversed.
//   codec   byword_codec<NS, true, log2 S> on the chosen codeword.
// Dynamic LDS: 4 S + 2 S + (4 or 8) bytes per symbol; states_list_max_symbols<S>() is the ONE place that says how long a word may be.
// Non-finite costs: dec keeps the path step's rules, every rank, position, state and candidate index stays in range, delta and
// choice are not specified.
template <int S, int NS>
struct StatesListShared : StatesStepShared<S, NS> {
    float delta[kListMaxT];
    float rho[64];
    __attribute__((aligned(4))) unsigned char raw[kRsRow];  // dec as bytes
    unsigned char order[64];                                // byte positions by rank
    __attribute__((aligned(4))) unsigned char cand[64 * kCandStride];
};

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

// The sweep and the walk: states_path_word with the survivors in `surv` and the metrics before every stage in `alpha`; the image is
// only read.  Leaves dec in dbits (and in `dec`, when wanted).
template <int S>
__device__ __forceinline__ void states_list_word(const float *image, float *alpha, unsigned *surv, int T, int lane,
                                                 unsigned char *dbits, float *__restrict__ dec) {
    using C = StatesCfg<S>;
    constexpr int LPB = C::LPB, R = C::R, TC = 8, WK = 32, H = S / 2;
    constexpr bool kWide = S > 32;  // the survivors of a stage take two dwords
    constexpr int SW = kWide ? 2 : 1;
    const int sl = lane % LPB;
    const int src0 = (2 * sl) % LPB, src1 = src0 + 1;
    float m = 0.0f;  // (128 states: a lane's two states end every stage with one value)
    auto load_chunk = [&](int t0, float (&c)[TC][R]) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) c[i][r] = image[(t0 + i) * S + sl + LPB * r];
    };
    float cur[TC][R], nxt[TC][R];
    load_chunk(0, nxt);
    for (int t0 = 0; t0 < T; t0 += TC) {
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) cur[i][r] = nxt[i][r];
        if (t0 + TC < T) load_chunk(t0 + TC, nxt);
#pragma unroll
        for (int i = 0; i < TC; ++i) {
            if (lane < H) alpha[(t0 + i) * H + lane] = m;  // the metric before stage t0 + i of states lane and lane + S / 2
            float a[R];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = m + -cur[i][r];
            float v0 = __shfl(a[0], src0), v1 = __shfl(a[0], src1);
            if (R == 2) {
                const float w0 = __shfl(a[R - 1], src0), w1 = __shfl(a[R - 1], src1);
                v0 = sl < 32 ? v0 : w0;
                v1 = sl < 32 ? v1 : w1;
            }
            const bool second = !(v1 >= v0) && v0 == v0;  // torch.min(dim): the first minimal index, the first NaN
            m = min2_torch_dev(v0, v1);
            const unsigned long long bal = __ballot(second);
            if (lane == 0) {
                surv[(t0 + i) * SW] = (unsigned)bal;
                if (kWide) surv[(t0 + i) * SW + SW - 1] = (unsigned)(bal >> 32);
            }
        }
    }
    wave_lds_fence();
    int s;
    {
        float bv = m;
        int bi = sl;
#pragma unroll
        for (int off = 1; off < LPB; off <<= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            const bool onan = ov != ov, bnan = bv != bv;
            const bool take = onan ? (!bnan || oi < bi) : (!bnan && ((ov < bv) || (ov == bv && oi < bi)));
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        s = __builtin_amdgcn_readfirstlane(bi);
    }
    // lane l's word of the 32 stages from `base`: stage base + (l & 31); a stage below 0 walks zeros, its bit is not stored
    auto fetch = [&](int base, unsigned &lo, unsigned &hi) {
        const int t = base + (lane & (WK - 1));
        lo = hi = 0u;
        if (t >= 0) {
            lo = surv[t * SW];
            if (kWide) hi = surv[t * SW + SW - 1];
        }
    };
    unsigned clo, chi, nlo, nhi;
    fetch(T - WK, clo, chi);
    for (int base = T - WK; base > -WK; base -= WK) {
        fetch(base - WK, nlo, nhi);
        unsigned path = 0;  // bit e: symbol base + e
#pragma unroll
        for (int e = WK - 1; e >= 0; --e) {
            unsigned w = (unsigned)__builtin_amdgcn_readlane((int)clo, e);
            if (kWide) {
                const unsigned wh = (unsigned)__builtin_amdgcn_readlane((int)chi, e);
                w = (s & 32) ? wh : w;
            }
            const int j = (int)(w >> (s & 31)) & 1;
            s = (2 * s + j) & (S - 1);
            path |= (unsigned)(s & 1) << e;
        }
        const int t = base + lane;
        if (lane < WK && t >= 0) {
            const int bit = (int)(path >> lane) & 1;
            dbits[t] = (unsigned char)bit;
            if (dec) dec[t] = (float)bit;
        }
        clo = nlo;
        chi = nhi;
    }
}

// Everything of the list step after the walk, by ONE wave: sh.dbits = dec, image = logit[t][S], alpha = the half-image [t][S / 2],
// sh.gf / sh.gen / sh.txrow as for byword_codec.  lo.ncand = C(lo.m, nsym).
template <int S, int NS>
__device__ __forceinline__ void states_list_tail(StatesListShared<S, NS> &sh, const float *image, float *alpha, int64_t r, int lane,
                                                 StepOut out, ListOut lo, int T, int nsym) {
    constexpr int H = S / 2, MEM = StatesCfg<S>::MEM;
    const int n = T >> 3, m = lo.m, ncand = lo.ncand;
    // ---- beta, and alpha + gamma in place: lane h (and every lane that repeats it) holds states h and h + S / 2
    {
        const int h = lane % H, src0 = h >> 1, src1 = src0 + H / 2;  // the lanes that hold gamma[p >> 1] of p = h and of p = h + S / 2
        float g = 0.0f;                                              // gamma_{t+1}; beta_T = 0
        float c0 = -image[(T - 1) * S + h], c1 = -image[(T - 1) * S + h + H], a = alpha[(T - 1) * H + h];
        for (int t = T - 1; t >= 0; --t) {
            const int tn = t > 0 ? t - 1 : 0;
            const float n0 = -image[tn * S + h], n1 = -image[tn * S + h + H], an = alpha[tn * H + h];  // the next step's operands, off the chain
            const float g0 = __shfl(g, src0), g1 = __shfl(g, src1);
            const float b0 = c0 + g0, b1 = c1 + g1;
            g = fminf(b0, b1);
            if (lane < H) alpha[t * H + h] = a + g;
            c0 = n0;
            c1 = n1;
            a = an;
        }
    }
    wave_lds_fence();
    // ---- delta, one lane per symbol; the lane's reads start at its own state so that the rows of a wave spread over the banks
    for (int t = lane; t < T; t += 64) {
        float mo = __builtin_inff(), me = __builtin_inff();
#pragma unroll 8
        for (int i = 0; i < H; ++i) {
            const int s = (i + lane) & (H - 1);
            const float v = alpha[t * H + s];
            if (s & 1) mo = fminf(mo, v);
            else me = fminf(me, v);
        }
        const float d = mo - me;
        sh.delta[t] = d;
        if (lo.delta) lo.delta[r * lo.delta_ld + t] = d;
    }
    wave_lds_fence();
    // ---- byte reliabilities and their order
    {
        float rho = __builtin_inff();
        if (lane < n) {
#pragma unroll
            for (int i = 0; i < 8; ++i) rho = fminf(rho, fabsf(sh.delta[8 * lane + i]));
        }
        sh.rho[lane] = rho;
        sh.order[lane] = (unsigned char)(lane < n ? lane : 0);  // (NaN reliabilities may leave ranks unassigned: still a byte of the word)
        wave_lds_fence();
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const float ri = sh.rho[i];
            rank += (ri < rho || (ri == rho && i < lane)) ? 1 : 0;
        }
        if (lane < n && rank < m) sh.order[rank] = (unsigned char)lane;
    }
    // ---- candidate 0: the hard decoder's codeword
    int synd[NS + 1];
    byword_decode_row<NS>(sh, lane, n, nsym, synd, sh.raw);
    byword_encode_row<NS>(sh, lane, n, nsym);
    for (int p = lane; p < n; p += 64) sh.cand[p] = sh.row[p];
    // ---- candidates 1 .. ncand, one per lane: unrank the subset, fill the erasures
    unsigned char *mine = sh.cand + lane * kCandStride;
    const bool valid = lane <= ncand;
    if (lane >= 1 && valid) {
        int pos[NS], mag[NS];
        int rem = lane - 1, x = 0;
#pragma unroll
        for (int l = 0; l < NS; ++l) {
            pos[l] = 0;
            if (l < nsym) {
                for (;;) {
                    const int cnt = list_binom(m - 1 - x, nsym - 1 - l);
                    if (rem < cnt || x >= m - 1) break;
                    rem -= cnt;
                    ++x;
                }
                pos[l] = sh.order[x];
                ++x;
            }
        }
        rs_erasure_fill<NS>(&sh.gf, synd, pos, n, nsym, mag);
        const unsigned int *src = reinterpret_cast<const unsigned int *>(sh.raw);
        unsigned int *dst = reinterpret_cast<unsigned int *>(mine);
        for (int w = 0; w < (n + 3) >> 2; ++w) dst[w] = src[w];
#pragma unroll
        for (int l = 0; l < NS; ++l)
            if (l < nsym) mine[pos[l]] ^= (unsigned char)mag[l];
    }
    wave_lds_fence();
    // ---- every candidate's own path through the branch costs
    float M = __builtin_inff();
    if (valid) {
        M = 0.0f;
        int nxt = mine[0];
        for (int jb = 0; jb < n; ++jb) {
            const int cur = nxt;
            nxt = jb + 1 < n ? mine[jb + 1] : 0;
            const unsigned w = (unsigned)((cur << 8) | nxt);  // b[8 jb] is bit 15
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned f = (w >> (16 - MEM - i)) & (unsigned)(S - 1);  // b[t] ... b[t + MEM - 1], b[t] highest
                const int st = (int)(__brev(f) >> (32 - MEM));                // its bits reversed: sum_i 2^i b[t + i]
                M = M + -image[(8 * jb + i) * S + st];
            }
        }
    }
    // ---- the smallest metric, the lowest index among equals (lane 0's view of the butterfly decides)
    int best = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oM = __shfl_xor(M, off);
        const int ob = __shfl_xor(best, off);
        if (oM < M || (oM == M && ob < best)) {
            M = oM;
            best = ob;
        }
    }
    best = __builtin_amdgcn_readfirstlane(best);
    if (best > ncand) best = 0;  // (only NaN metrics can leave an unused lane's index here)
    if (lane == 0 && lo.choice) lo.choice[r] = best;
    if (best != 0)
        for (int p = lane; p < n; p += 64) sh.row[p] = sh.cand[best * kCandStride + p];
    wave_lds_fence();
    byword_codec<NS, true, MEM>(sh, r, lane, out, T, nsym, 0);
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
    {
        // ---- phase 1: the word's tiles, round-robin over the waves
        const int j = lane & 15, q = lane >> 4;
        const float *rxb = rx + r * rx_ld;
        mlp_stage_w3<C::NT3>(sh.a3, sh.b3, W3 + r * ws.s[4], b3 + r * ws.s[5], S);
        float nw1[kK2Steps], nb1[kK2Steps], a2[4][kK2Steps], b2v[4][4];
        mlp_load_weights(W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2], b2 + r * ws.s[3], j, q, nw1, nb1, a2, b2v);
        __syncthreads();
        const int ntiles = (T + 15) >> 4;
        for (int tile = wave; tile < ntiles; tile += kStatesWaves) {
            const int t = 16 * tile + j;
            const float yj = rxb[t < T ? t : T - 1];
            mlp_tile<C::NT3>(yj, nw1, nb1, a2, b2v, sh.a3, lane, [&](int j3, f32x4 acc3) {
                const int st0 = 16 * j3 + 4 * q;
                if (st0 < S && t < T) {
                    float4 v;
                    v.x = acc3[0] + sh.b3[st0 + 0];
                    v.y = acc3[1] + sh.b3[st0 + 1];
                    v.z = acc3[2] + sh.b3[st0 + 2];
                    v.w = acc3[3] + sh.b3[st0 + 3];
                    *reinterpret_cast<float4 *>(&states_logit[t * S + st0]) = v;
                }
            });
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- phase 2: wave 0 sweeps the word, walks its survivors back, list-decodes and carries on with the codec
    float *alpha = states_logit + T * S;
    unsigned *surv = reinterpret_cast<unsigned *>(alpha + T * (S / 2));
    states_list_word<S>(states_logit, alpha, surv, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the workgroup barrier: tables complete)
    wave_lds_fence();
    states_list_tail<S, NS>(sh, states_logit, alpha, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out},
                            {delta_out, delta_ld, choice_out, m, ncand}, T, nsym);
}
