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

// Everything of a block step after the detection, by ONE wave (the caller's): sh.dbits holds the detected word (data step),
// sh.txrow the transmitted message as bytes, sh.gf the tables (and sh.gen the generator polynomial when NS > 2); word r's
// outputs as in mvn_vnet_byword_step_f32.
template <int NS>
__device__ __forceinline__ void byword_codec(StepShared<NS> &sh, int64_t r, int lane, float *__restrict__ msg, int64_t msg_ld,
                                             float *__restrict__ enc, int64_t enc_ld, float *__restrict__ label_word, int64_t lw_ld,
                                             int *__restrict__ labels, int64_t lab_ld, int *__restrict__ nerr_out, int T, int nsym,
                                             int pilot) {
    constexpr bool kClosedForm = NS <= 2;  // parity from the message's sums at 2^0, 2^1 instead of the generator polynomial
    GfTables &gf = sh.gf;
    int *gen = sh.gen, *s_loc = sh.s_loc;
    unsigned char *row = sh.row, *txrow = sh.txrow, *dbits = sh.dbits, *lwb = sh.lwb;
    const int n = T >> 3, k = n - nsym;
    // ---- one wave (the deciding wave; wave 0 on a pilot): the codec on the word's byte image
    int nerr = 0;
    if (!pilot) {
        // np.packbits of the detected word, one lane per byte; syndromes synd[i + 1] = sum_p byte_p (2^i)^(n - 1 - p)
        // (rs_calc_syndromes, rs_decoder.py:37-47, Horner form written out), xor-reduced over the lanes
        int synd[NS + 1];
        synd[0] = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) synd[i + 1] = 0;
        for (int p = lane; p < n; p += 64) {
            int byte = 0;
#pragma unroll
            for (int jb = 0; jb < 8; ++jb) byte = (byte << 1) | (dbits[8 * p + jb] & 1);
            row[p] = (unsigned char)byte;
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
        for (int p = lane; p < k; p += 64) nerr += __popc((unsigned)(row[p] ^ txrow[p]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) nerr += __shfl_xor(nerr, off);
        if (msg) {
            float *mb = msg + r * msg_ld;
            for (int e = lane; e < 8 * k; e += 64) mb[e] = (float)((row[e >> 3] >> (7 - (e & 7))) & 1);
        }
    } else {
        for (int p = lane; p < k; p += 64) row[p] = txrow[p];
    }
    if (lane == 0 && nerr_out) nerr_out[r] = nerr;
    if (!enc && !label_word && !labels) return;  // (the evaluation without updates reads the error count only)
    wave_lds_fence();
    // encode(decoded) / encode(transmitted)  (rs_encoder.py:7-37)
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
        rs_append_parity<NS>(gf, gen, row, k, nsym);
    }
    wave_lds_fence();

    // ---- encoded word, label word (trainer.py:322-324) and its trellis states
    const bool use_detected = nerr > 0;
    float *eb = enc ? enc + r * enc_ld : nullptr, *lb = label_word ? label_word + r * lw_ld : nullptr;
    for (int t = lane; t < T + kStepMemory; t += 64) {
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
    if (labels) {
        int *lab = labels + r * lab_ld;
        for (int t = lane; t < T; t += 64) {
            int st = 0;
#pragma unroll
            for (int i = 0; i < kStepMemory; ++i) st |= (int)lwb[t + i] << i;  // state[t] = sum_i 2^i b[t + i]
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
    byword_codec<NS>(sh, r, lane, msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out, T, nsym, pilot);
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
    byword_codec<NS>(sh, r, lane, msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out, T, nsym, pilot);
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
    byword_codec<NS>(sh, r, lane, msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out, T, nsym, 0);
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
    byword_codec<NS>(sh, r, lane, msg, msg_ld, enc, enc_ld, label_word, lw_ld, labels, lab_ld, nerr_out, T, nsym, 0);
}
