// byword_step.inc -- one block step of the by-word evaluation in ONE launch (included by mvn_hip.hip after vnet16_coop.inc
// and rs_codec.inc).
//
// Counterpart of the per-block body of Trainer.eval_by_word (python_code/trainers/trainer.py:292-316) for the 16-state
// ViterbiNet detector with the Reed-Solomon outer code:
//     detected = detector(rx, 'val')                          (:295)
//     data block : decoded = RS-decode(detected); errors vs the transmitted word; encoded = RS-encode(decoded)   (:298-304)
//     pilot block: encoded = RS-encode(transmitted)           (:314-316; the detection of a pilot is never used)
//     label word = detected if the block has bit errors else encoded          (:322-324, what the buffer stores)
// and calculate_states (utils/trellis_utils.py:33-46) of the label word, which is all the training kernels ever read of it.
// The reference (and rounds 1-2 of this library) issue four launches and a host round trip per block; here a 16-wave
// workgroup per word runs vnet16_coop's detector (same arithmetic: bit-identical decisions), and the wave that made the
// decisions continues with the codec on an LDS byte image of the word: syndromes in parallel over the bytes (one lane per
// byte, xor butterfly); only when a syndrome is non-zero Berlekamp-Massey by one lane, the exhaustive root search one
// position per lane, Forney by one lane; the error count against the transmitted message by byte-wise popcounts; the parity
// bytes in closed form from two more parallel sums when nsym <= 2 (the code is MDS: the codeword with the given message part
// that vanishes at 2^0 and 2^1 is the systematic encoder's), else by one lane's synthetic division.  A lone lane's table
// look-ups are dependent LDS round trips: the serial parts are what a B = 1 step waits for.
// gridDim.x = R words, each with ITS OWN weights (word r uses W + r * stride): R independent trials of the evaluation
// advance one block per launch (harness.eval_by_word_batched); R = 1 is the reference's sequential call pattern.
//
// The family is two detectors times three decision rules (StepDecision): six kernels here, twelve with NS = 2 and 8, and the three
// of byword_step_states.inc / byword_list_states.inc at five more state counts.  They share the codec, byword_list_tail (ONE copy for
// every state count: what differs off 16 states is chosen by if constexpr inside it), ListFields, the detectors and path16_walk as code,
// and StepOut / ListOut as types: a kernel packs its output parameters where it calls the codec or the list tail.  The structs travel
// BY VALUE and each kernel keeps its own staging, detection and finish lines and its LDS in the __global__ function: a const reference
// to the structs, a reference to the LDS object in a shared staging or finish function, or one more forceinline layer around a
// kernel's lines each change what the compiler emits for it (the traced-back kernels then measure 1-2 % slower).  Share more here only
// with an unchanged disassembly of every by-word kernel, at every instantiation.  To check it, build the device assembly of the parent
// commit and of the tree with the library's flags (__graft_entry__.py: HIPCC_FLAGS without -shared -fPIC) and compare them:
//     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S mvn_hip.hip -o tree.s     (parent.s alike)
//     python tools/kernel_isa_diff.py parent.s tree.s        ("same N diff 0"; once more with -DMVN_TEST_HOOKS)
// profiles/byword_isa_identity.txt holds that output for the change that made the list tail and the sweep-and-walk one copy each.
struct WeightStrides {
    long long s[6];  // elements between consecutive words' W1, b1, W2, b2, W3, b3 (0: all words share one set)
};

constexpr int kStepMemory = 4;  // memory_length of the 16-state trellis

// LDS of a block step: codec tables, the word's byte images, the decisions as bits
template <int NS>
struct StepShared {
    GfTables gf;
    int gen[NS + 1];
    unsigned char row[kRsRow], txrow[kRsRow];
    unsigned char dbits[kCoopMaxT], lwb[kCoopMaxT + 16];
    int s_loc[NS + 4];  // the error locator and its {length, leading zeros}, from the lane that ran Berlekamp-Massey
};

enum StepDecision { kStepRunning, kStepPath, kStepList };  // what the codec is fed: running-argmin decisions, the traced-back path, its list decode
// What a step writes for word r, as in mvn_vnet_byword_step_f32, and the list step's own outputs and limits, as in
// mvn_vnet_byword_step_list_f32 (an output pointer that is NULL: not wanted).  The kernels pack them from their parameters.
struct StepOut {
    float *msg; int64_t msg_ld;
    float *enc; int64_t enc_ld;
    float *label_word; int64_t lw_ld;
    int *labels; int64_t lab_ld;
    int *nerr;
};
struct ListOut {
    float *delta; int64_t delta_ld;
    int *choice;
    int m, ncand;  // list_bytes and C(m, nsym)
};

// The hard decoder of a data step, by ONE wave: np.packbits of sh.dbits into sh.row (and into raw, when given: the word's bytes as
// detected), the syndromes (left in synd, every lane alike), and the correction of the message bytes in place.
template <int NS>
__device__ __forceinline__ void byword_decode_row(StepShared<NS> &sh, int lane, int n, int nsym, int (&synd)[NS + 1],
                                                  unsigned char *raw) {
    GfTables &gf = sh.gf;
    int *s_loc = sh.s_loc;
    unsigned char *row = sh.row, *dbits = sh.dbits;
    // np.packbits of the detected word, one lane per byte; syndromes synd[i + 1] = sum_p byte_p (2^i)^(n - 1 - p)
    // (rs_calc_syndromes, rs_decoder.py:37-47, Horner form written out), xor-reduced over the lanes
    synd[0] = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) synd[i + 1] = 0;
    for (int p = lane; p < n; p += 64) {
        int byte = 0;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) byte = (byte << 1) | (dbits[8 * p + jb] & 1);
        row[p] = (unsigned char)byte;
        if (raw) raw[p] = (unsigned char)byte;
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < nsym) synd[i + 1] ^= gf_mul(&gf, byte, gf_pow2(&gf, i * (n - 1 - p)));
    }
    int any = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) synd[i + 1] ^= __shfl_xor(synd[i + 1], off);
        any |= synd[i + 1];
    }
    wave_lds_fence();
    if (any) {  // wave-uniform: rs_locate_correct's three stages, the middle one spread over the lanes
        if (lane == 0) {
            int err_loc[NS + 2], lead;
            const int el = rs_error_locator<NS>(&gf, synd, nsym, err_loc, lead);
            for (int t = 0; t < el; ++t) s_loc[t] = err_loc[t];
            s_loc[NS + 2] = el;
            s_loc[NS + 3] = lead;
        }
        wave_lds_fence();
        const int el = s_loc[NS + 2], lead = s_loc[NS + 3];
        if ((el - lead - 1) * 2 <= nsym) {  // else "too many errors": the uncorrected systematic part (rs_main.py:31-33)
            // rs_find_errors: position n - 1 - i errs iff the locator vanishes at 2^i; kept in the order of i
            unsigned long long roots[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = lane + 64 * h;
                roots[h] = __ballot(i < n && rs_locator_at(&gf, s_loc, el, lead, i) == 0);
            }
            if (lane == 0) {
                int npos = 0, pos[NS / 2 + 1];
                for (int h = 0; h < 2; ++h)
                    for (unsigned long long m = roots[h]; m && npos <= NS / 2; m &= m - 1)
                        pos[npos++] = n - 1 - (64 * h + __builtin_ctzll(m));
                rs_forney_correct<NS>(&gf, synd, pos, npos, row, n, nsym);
            }
        }
    }
    wave_lds_fence();
}

// encode(message bytes sh.row[0 .. k)) by ONE wave: the parity bytes sh.row[k .. n)  (rs_encoder.py:7-37)
template <int NS>
__device__ __forceinline__ void byword_encode_row(StepShared<NS> &sh, int lane, int n, int nsym) {
    constexpr bool kClosedForm = NS <= 2;  // parity from the message's sums at 2^0, 2^1 instead of the generator polynomial
    GfTables &gf = sh.gf;
    unsigned char *row = sh.row;
    const int k = n - nsym;
    if (kClosedForm) {
        int s0 = 0, s1 = 0;  // the message part at 2^0 and 2^1
        for (int p = lane; p < k; p += 64) {
            const int byte = row[p];
            s0 ^= byte;
            s1 ^= gf_mul(&gf, byte, gf_pow2(&gf, n - 1 - p));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s0 ^= __shfl_xor(s0, off);
            s1 ^= __shfl_xor(s1, off);
        }
        if (lane == 0) {
            if (nsym == 1) {
                row[k] = (unsigned char)s0;  // c(1) = 0
            } else {  // c(1) = c(2) = 0 for c = message . x^2 + r0 x + r1:  r0 = (s0 + s1) / (1 + 2),  r1 = s0 + r0
                const int r0 = gf_div(&gf, s0 ^ s1, 3);
                row[k] = (unsigned char)r0;
                row[k + 1] = (unsigned char)(s0 ^ r0);
            }
        }
    } else if (lane == 0) {
        rs_append_parity<NS>(gf, sh.gen, row, k, nsym);
    }
    wave_lds_fence();
}

// Everything of a block step after the detection, by ONE wave (the caller's): sh.dbits holds the detected word (data step),
// sh.txrow the transmitted message as bytes, sh.gf the tables (and sh.gen the generator polynomial when NS > 2); word r's
// outputs as in mvn_vnet_byword_step_f32.  CHOSEN (the list step, below): sh.row already holds the codeword to report.
// MEM: the memory length of the trellis whose states label the word (byword_step_states.inc: log2 of its state count).
template <int NS, bool CHOSEN = false, int MEM = kStepMemory>
__device__ __forceinline__ void byword_codec(StepShared<NS> &sh, int64_t r, int lane, StepOut out, int T, int nsym, int pilot) {
    unsigned char *row = sh.row, *txrow = sh.txrow, *dbits = sh.dbits, *lwb = sh.lwb;
    const int n = T >> 3, k = n - nsym;
    // ---- one wave (the deciding wave; wave 0 on a pilot): the codec on the word's byte image
    int nerr = 0;
    if (!pilot) {
        if (!CHOSEN) {
            int synd[NS + 1];
            byword_decode_row<NS>(sh, lane, n, nsym, synd, nullptr);
        }
        for (int p = lane; p < k; p += 64) nerr += __popc((unsigned)(row[p] ^ txrow[p]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nerr += __shfl_xor(nerr, off);
        if (out.msg) {
            float *mb = out.msg + r * out.msg_ld;
            for (int e = lane; e < 8 * k; e += 64) mb[e] = (float)((row[e >> 3] >> (7 - (e & 7))) & 1);
        }
    } else {
        for (int p = lane; p < k; p += 64) row[p] = txrow[p];
    }
    if (lane == 0 && out.nerr) out.nerr[r] = nerr;
    if (!out.enc && !out.label_word && !out.labels) return;  // (the evaluation without updates reads the error count only)
    wave_lds_fence();
    if (!CHOSEN) byword_encode_row<NS>(sh, lane, n, nsym);  // encode(decoded) / encode(transmitted)

    // ---- encoded word, label word (trainer.py:322-324) and its trellis states
    const bool use_detected = nerr > 0;
    float *eb = out.enc ? out.enc + r * out.enc_ld : nullptr, *lb = out.label_word ? out.label_word + r * out.lw_ld : nullptr;
    for (int t = lane; t < T + MEM; t += 64) {
        int ebit = 0, lbit = 0;
        if (t < T) {
            ebit = (row[t >> 3] >> (7 - (t & 7))) & 1;
            lbit = use_detected ? (dbits[t] & 1) : ebit;
            if (eb) eb[t] = (float)ebit;
            if (lb) lb[t] = (float)lbit;
        }
        lwb[t] = (unsigned char)lbit;  // zero padding by the memory length (channel_dataset.py:71)
    }
    wave_lds_fence();
    if (out.labels) {
        int *lab = out.labels + r * out.lab_ld;
        for (int t = lane; t < T; t += 64) {
            int st = 0;
#pragma unroll
            for (int i = 0; i < MEM; ++i) st |= (int)lwb[t + i] << i;  // state[t] = sum_i 2^i b[t + i]
            lab[t] = st;
        }
    }
}

template <int NS>
__global__ __launch_bounds__(64 * kCoopWaves, 4) void byword_step_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    __shared__ StepShared<NS> sh;
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = T >> 3, k = n - nsym;

    // side work of the waves that have no MLP tile (or, on a pilot, of everyone): codec tables, generator polynomial,
    // the transmitted message as bytes
    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    if (pilot) {
        __syncthreads();
        if (wave != 0) return;
        if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    } else {
        float *decb = dec ? dec + r * dec_ld : nullptr;
        float m_unused;
        unsigned char *dbits = sh.dbits;
        const int role = coop_detect_block<false>(rx + r * rx_ld, W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2],
                                                  b2 + r * ws.s[3], W3 + r * ws.s[4], b3 + r * ws.s[5], nullptr, T, &m_unused,
                                                  [&](int tdec, float mydec, bool live) {
                                                      if (!live) return;
                                                      if (decb) decb[tdec] = mydec;
                                                      dbits[tdec] = (unsigned char)mydec;
                                                  });
        if (role != kCoopDecided) return;  // the wave that made the decisions carries on with the codec
        if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);  // (after the detector's workgroup barrier: tables complete)
    }
    wave_lds_fence();
    byword_codec<NS>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}

// The same block step for the CLASSICAL Viterbi detector at 16 states (the reference's eval_by_word takes any detector,
// trainer.py:295; golden G9 is a VA by-word run): ONE wave per word -- va16_tile.inc's detector (a lone sweeping wave: the
// branch costs need no MLP, so there is nothing for other waves to do), then the codec above.  Word r uses row r % Bp of the
// state priors (VADetector.compute_state_priors: one row per word's channel, or one for all).
template <int NS>
__global__ __launch_bounds__(64) void byword_step_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym, int pilot) {
    __shared__ StepShared<NS> sh;
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int n = T >> 3, k = n - nsym;
    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = lane; p < k; p += 64) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    if (!pilot) {
        float *decb = dec ? dec + r * dec_ld : nullptr;
        unsigned char *dbits = sh.dbits;
        va16_tile_block(rx + r * rx_ld, priors + (r % Bp) * 16, T, [&](int t, float mydec) {
            if (decb) decb[t] = mydec;
            dbits[t] = (unsigned char)mydec;
        });
    }
    wave_lds_fence();  // (one wave: its own LDS writes -- tables, bytes, decisions -- are visible to all its lanes)
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    wave_lds_fence();
    byword_codec<NS>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, pilot);
}

// ---- The block step on the TRACED-BACK PATH (mvn_vnet_byword_step_path_f32 / mvn_va_byword_step_path_f32).  The steps above feed
// the codec with the reference's running-argmin decisions (quirk Q1: symbol t is decided before stage t is absorbed); these feed
// it with the textbook maximum-likelihood word -- the survivors of mvn_*_decode_surv_f32 walked back as mvn_traceback_f32 walks
// them -- and change nothing else: the survivor words of the block stay in LDS (2 B per symbol, vnet16_common.inc's per-lane form),
// one wave walks them from registers and carries on into byword_codec with the path's bits in sh.dbits.
template <int NS>
struct PathStepShared : StepShared<NS> {
    __attribute__((aligned(16))) unsigned short surv[kCoopMaxT];
    float fm[16];  // the final path metric, logical state order
};

template <int NS>
__global__ __launch_bounds__(64 * kCoopWaves, 4) void byword_path_step_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym) {
    __shared__ PathStepShared<NS> sh;
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = (T >> 3) - nsym;
    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    float m_unused;
    const int role = coop_detect_block<false, true>(rx + r * rx_ld, W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2],
                                                    b2 + r * ws.s[3], W3 + r * ws.s[4], b3 + r * ws.s[5], nullptr, T, &m_unused,
                                                    [](int, float, bool) {}, sh.surv, sh.fm);
    if (role != kCoopDecided) return;  // the wave that formed the survivors walks them back and carries on with the codec
    path16_walk(sh.surv, sh.fm, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    wave_lds_fence();
    byword_codec<NS>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}

template <int NS>
__global__ __launch_bounds__(64) void byword_path_step_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, int T, int nsym) {
    __shared__ PathStepShared<NS> sh;
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = (T >> 3) - nsym;
    gf_load(&sh.gf);
    {
        const float *txb = tx + r * tx_ld;
        for (int p = lane; p < k; p += 64) sh.txrow[p] = (unsigned char)pack_byte(txb + 8 * p);
    }
    va16_tile_block_surv(rx + r * rx_ld, priors + (r % Bp) * 16, T, sh.surv, sh.fm);
    path16_walk(sh.surv, sh.fm, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    wave_lds_fence();
    byword_codec<NS>(sh, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out}, T, nsym, 0);
}

// ---- The block step with a RELIABILITY-ORDERED LIST DECODE (mvn_vnet_byword_step_list_f32 / mvn_va_byword_step_list_f32).  The path
// step above hands the hard decoder the traced-back word dec and throws the rest of the trellis away; here the branch costs
// cost[t][s] (s = the state before stage t) and the forward metrics alpha_t[s] stay in LDS, and the wave that walked the path back
// goes on, everything in fp32 with individually rounded operations:
//   beta    beta_T = 0, beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | 8]), one lane per state (16 lanes);
//           alpha_t + beta_t overwrites the alpha image
//   delta   delta_t = min_{s odd}(alpha_t[s] + beta_t[s]) - min_{s even}(...), the max-log LLR, one lane per symbol
//   rank    rho_j = min_{i<8} |delta_{8j+i}|; the n = T / 8 bytes ordered by (rho, j); U = the first m of them
//   cand 0  the hard decoder's message for dec (byword_decode_row, as the path step) and its parity
//   cand c  c = 1 .. C(m, nsym), ONE PER LANE: the c-th nsym-subset of U in lexicographic order of ranks is erased in dec and filled
//           (rs_erasure_fill)
//   metric  M(c) = sum_t cost[t][state_t(c)] in ascending t, state_t = sum_i 2^i b[t + i] of the candidate codeword padded with zeros
//   choice  the smallest M, the lowest index among equals; that codeword is what the rest of the step (byword_codec) reports
// T <= kListMaxT = 512: costs and alpha take 64 B per symbol each, 64 KB at T = 512 next to the ViterbiNet workgroup's 57.6 KB of
// weights, tiles and step state (121.6 KB of a CU's 160 KB); T = 1024 would need 128 KB, which no CU has next to them.
// Non-finite costs: candidate 0 keeps the path step's rules; ranks, fills and the choice are then deterministic and every index stays
// in range, but which candidate wins is not specified.
constexpr int kListMaxT = 512;
constexpr int kListMaxCand = 63;    // candidates 1 .. 63 next to the hard decoder's: one wave
constexpr int kCandStride = 68;     // bytes between the candidates' codewords: 17 dwords, the lanes' byte reads spread over the banks

// The list's own LDS, ONCE, on top of the step it extends: ListStepShared<NS> at 16 states, StatesListShared<S, NS>
// (byword_list_states.inc) at the other state counts.
template <class Base>
struct ListFields : Base {
    float delta[kListMaxT];
    float rho[64];
    __attribute__((aligned(4))) unsigned char raw[kRsRow];  // dec as bytes
    unsigned char order[64];                                // byte positions by rank
    __attribute__((aligned(4))) unsigned char cand[64 * kCandStride];
};
template <int NS>
using ListStepShared = ListFields<PathStepShared<NS>>;

__device__ __forceinline__ int list_binom(int a, int b) {  // C(a, b), every partial product a binomial itself
    if (b < 0 || b > a) return 0;
    int c = 1;
    for (int i = 1; i <= b; ++i) c = c * (a - b + i) / i;
    return c;
}

// Everything of a list step after the walk, by ONE wave, at every state count: sh.dbits = dec, sh.gf / sh.gen / sh.txrow as for
// byword_codec.  lo.ncand = C(lo.m, nsym).  S = 16: cost / alpha = the [t][16] images.  Any other S (byword_list_states.inc, which
// states the forms): cost = the LOGIT image [t][S] (cost = -logit), alpha = the half-image [t][S / 2].  Three pieces differ with S, each
// as its family had it: the beta recursion, the delta loop, the candidate's state and cost look-up; everything else is one copy.
template <int NS, int S = 16, class Shared>
__device__ __forceinline__ void byword_list_tail(Shared &sh, const float *cost, float *alpha, int64_t r, int lane, StepOut out,
                                                 ListOut lo, int T, int nsym) {
    constexpr int H = S / 2, MEM = __builtin_ctz(S);
    const int n = T >> 3, m = lo.m, ncand = lo.ncand;
    if constexpr (S == 16) {
        // ---- beta, and alpha + beta in place: lanes 0..15, one per state (the other lanes take part in the cross-lane reads only;
        // what they hold is never read)
        const int s = lane & 15, src0 = s >> 1, src1 = src0 | 8;
        const bool mine = lane < 16;
        float beta = 0.0f;
        float c = mine ? cost[(T - 1) * 16 + s] : 0.0f, a = mine ? alpha[(T - 1) * 16 + s] : 0.0f;
        for (int t = T - 1; t >= 0; --t) {
            const int tn = t > 0 ? t - 1 : 0;
            float cn = 0.0f, an = 0.0f;
            if (mine) {  // the next step's operands, off the chain
                cn = cost[tn * 16 + s];
                an = alpha[tn * 16 + s];
            }
            const float b0 = __shfl(beta, src0), b1 = __shfl(beta, src1);
            beta = c + fminf(b0, b1);
            if (mine) alpha[t * 16 + s] = a + beta;
            c = cn;
            a = an;
        }
    } else {
        // ---- beta, and alpha + gamma in place: lane h (and every lane that repeats it) holds states h and h + S / 2
        const int h = lane % H, src0 = h >> 1, src1 = src0 + H / 2;  // the lanes that hold gamma[p >> 1] of p = h and of p = h + S / 2
        float g = 0.0f;                                              // gamma_{t+1}; beta_T = 0
        float c0 = -cost[(T - 1) * S + h], c1 = -cost[(T - 1) * S + h + H], a = alpha[(T - 1) * H + h];
        for (int t = T - 1; t >= 0; --t) {
            const int tn = t > 0 ? t - 1 : 0;
            const float n0 = -cost[tn * S + h], n1 = -cost[tn * S + h + H], an = alpha[tn * H + h];  // the next step's operands, off the chain
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
        if constexpr (S == 16) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int s = (i + lane) & 15;
                const float v = alpha[t * 16 + s];
                if (s & 1) mo = fminf(mo, v);
                else me = fminf(me, v);
            }
        } else {
#pragma unroll 8
            for (int i = 0; i < H; ++i) {
                const int s = (i + lane) & (H - 1);
                const float v = alpha[t * H + s];
                if (s & 1) mo = fminf(mo, v);
                else me = fminf(me, v);
            }
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
            if constexpr (S == 16) {
                const int w = (cur << 8) | nxt;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int nib = (w >> (12 - i)) & 15;                              // b[t] b[t+1] b[t+2] b[t+3], b[t] highest
                    const int st = (int)((0xF7B3D591E6A2C480ull >> (4 * nib)) & 15);  // its bits reversed: sum_i 2^i b[t + i]
                    M = M + cost[(8 * jb + i) * 16 + st];
                }
            } else {
                const unsigned w = (unsigned)((cur << 8) | nxt);  // b[8 jb] is bit 15
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned f = (w >> (16 - MEM - i)) & (unsigned)(S - 1);  // b[t] ... b[t + MEM - 1], b[t] highest
                    const int st = (int)(__brev(f) >> (32 - MEM));                // its bits reversed: sum_i 2^i b[t + i]
                    M = M + -cost[(8 * jb + i) * S + st];
                }
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

template <int NS>
__global__ __launch_bounds__(64 * kCoopWaves, 4) void byword_list_step_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ W1,
    const float *__restrict__ b1, const float *__restrict__ W2, const float *__restrict__ b2, const float *__restrict__ W3,
    const float *__restrict__ b3, WeightStrides ws, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg,
    int64_t msg_ld, float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
    int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, float *__restrict__ delta_out, int64_t delta_ld,
    int *__restrict__ choice_out, int T, int nsym, int m, int ncand) {
    __shared__ ListStepShared<NS> sh;
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = (T >> 3) - nsym;
    gf_load(&sh.gf);
    {
        const float *txb = tx ? tx + r * tx_ld : nullptr;  // (no transmitted word: a decoder, nothing is counted)
        for (int p = blockDim.x - 1 - threadIdx.x; p < k; p += blockDim.x)
            sh.txrow[p] = txb ? (unsigned char)pack_byte(txb + 8 * p) : (unsigned char)0;
    }
    float m_unused;
    float *alpha = nullptr;
    const int role = coop_detect_block<false, true, true>(rx + r * rx_ld, W1 + r * ws.s[0], b1 + r * ws.s[1], W2 + r * ws.s[2],
                                                          b2 + r * ws.s[3], W3 + r * ws.s[4], b3 + r * ws.s[5], nullptr, T, &m_unused,
                                                          [](int, float, bool) {}, sh.surv, sh.fm, &alpha);
    if (role != kCoopDecided) return;
    path16_walk(sh.surv, sh.fm, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    wave_lds_fence();
    byword_list_tail<NS>(sh, alpha - ((T + 15) >> 4) * 256, alpha, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out},
                         {delta_out, delta_ld, choice_out, m, ncand}, T, nsym);
}

template <int NS>
__global__ __launch_bounds__(64) void byword_list_step_va_kernel(
    const float *__restrict__ rx, int64_t rx_ld, const float *__restrict__ tx, int64_t tx_ld, const float *__restrict__ priors,
    int64_t Bp, float *__restrict__ dec, int64_t dec_ld, float *__restrict__ msg, int64_t msg_ld, float *__restrict__ enc,
    int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld, int *__restrict__ labels, int64_t lab_ld,
    int *__restrict__ nerr_out, float *__restrict__ delta_out, int64_t delta_ld, int *__restrict__ choice_out, int T, int nsym,
    int m, int ncand) {
    __shared__ ListStepShared<NS> sh;
    extern __shared__ float va_list_img[];  // cost[t][16], then alpha[t][16], 16 * ceil(T / 16) rows each
    constexpr bool kClosedForm = NS <= 2;
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int k = (T >> 3) - nsym;
    float *cost = va_list_img, *alpha = va_list_img + ((T + 15) >> 4) * 256;
    gf_load(&sh.gf);
    {
        const float *txb = tx ? tx + r * tx_ld : nullptr;
        for (int p = lane; p < k; p += 64) sh.txrow[p] = txb ? (unsigned char)pack_byte(txb + 8 * p) : (unsigned char)0;
    }
    va16_tile_block_surv<true>(rx + r * rx_ld, priors + (r % Bp) * 16, T, sh.surv, sh.fm, cost, alpha);
    path16_walk(sh.surv, sh.fm, T, lane, sh.dbits, dec ? dec + r * dec_ld : nullptr);
    if (!kClosedForm && lane == 0) rs_generator_poly<NS>(sh.gf, sh.gen, nsym);
    wave_lds_fence();
    byword_list_tail<NS>(sh, cost, alpha, r, lane, {msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out},
                         {delta_out, delta_ld, choice_out, m, ncand}, T, nsym);
}
