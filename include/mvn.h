/*
 * mvn.h -- C ABI of libmvn_hip.so: the MI355X (gfx950) Viterbi / ViterbiNet detection engine.
 *
 * This is the drop-in boundary for the 'val' hot path of tomerraviv95/meta-viterbinet.
 * The reference has no FFI of its own (pure Python); each entry point below
 * replaces the body of one reference function and is what a ctypes stub in the reference's
 * detector modules would bind (INTEGRATION.md shows that stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all memory;
 *   - fp32 row-major; `*_ld` = row stride in elements; S = n_states = 2**memory_length,
 *     a power of two in [2,256] (the reference's np.uint8 bound, va_detector.py:43);
 *   - pointers need their type's natural alignment only (4 bytes for fp32); 16-byte aligned
 *     buffers and row strides that are multiples of 4 get the vector load/store paths;
 *   - calls enqueue work on `stream` (a hipStream_t; NULL = default stream) and return
 *     immediately: they never allocate, free or synchronise, so they can be graph-captured;
 *   - what a capture FREEZES: a captured call replays the launches it issued with the arguments it issued them with.  Device
 *     buffers are read anew by every replay (samples, weights, priors, optimizer moments, device-side descriptors such as the
 *     trial entry points' b1pow / b2pow); everything the HOST worked out at capture time is not:
 *       . host scalars passed by value: step counts (step0) and the powers of beta1 / beta2 the training entry points derive
 *         from them (an Adam replay repeats the bias correction of the captured step0; SGD and RMSprop steps do not depend
 *         on it), seeds and word0 of the Monte-Carlo and word-generator calls (a replay draws the same words again), lr, snr;
 *       . the MVN_* switches as they stood at capture (mvn_reload_switches has no effect on a captured graph);
 *       . the choice of kernel, made from B, T, S, pointer alignment, workspace size and the device's CU count.
 *     A workspace (and its status word) belongs to one call at a time: a captured call's workspace must not be shared with
 *     work that may run concurrently with a replay, other replays of the same graph included.  Under capture the calls that
 *     use the dealt 16-state kernel put one memset node (the hand-off lines) in front of the kernel; outside capture they
 *     issue the kernel alone;
 *   - return value: 0 = ok, <0 = bad argument (MVN_E_*), >0 = hipError_t of the failed launch.
 *   - decisions are written as fp32 {0.,1.} like the reference's decoded_word
 *     (va_detector.py:90-93); columns >= T of `dec` are not touched (caller zero-fills).
 *   - arithmetic is IEEE fp32 with one rounding per reference operation; results are
 *     bit-identical to oracle/mvn_oracle.c for finite inputs, for +-inf, and for NaN -- in the samples y, in the weights
 *     and in the state priors: mvn_acs_block_f32, mvn_va_decode_f32, mvn_vnet_decode_f32 (every route, every S),
 *     mvn_acs_sweep_f32, mvn_vnet_decode_count_f32 and mvn_vnet_byword_step_f32 follow torch.min / torch.argmin (NaN when
 *     either candidate is NaN; the first NaN, else the first minimum).  The fast kernels' ACS stage is v_min_f32 (minNum),
 *     which agrees with torch.min unless SOME BUT NOT ALL of a symbol's branch costs are NaN (or +inf meets -inf in a path
 *     metric).  From y, weights and priors that takes a non-finite (or > 1e14 in magnitude) weight or prior, which the kernels
 *     look for once per launch and then run their NaN-propagating form (16-state kernels) or are followed by a guard launch of
 *     the generic kernel that re-decodes the affected blocks (sweep_kernel<S, MODE, true>: an early-exit no-op otherwise).
 *     MATERIALISED costs (mvn_acs_sweep_f32; the logits of the two-kernel ViterbiNet route) are tested one by one on their way
 *     into the recurrence: from the first cost that is NaN, infinite or >= 1e30 in magnitude on, a wave runs the
 *     NaN-propagating stage and decision.
 */
#ifndef MVN_H_
#define MVN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mvn_stream_t; /* hipStream_t */

#define MVN_OK 0
#define MVN_E_DIMS (-1)      /* negative size, T > ld, a non-Adam optimizer tag for the meta-learning calls, ... */
#define MVN_E_STATES (-2)    /* S not a power of two in [2,256] */
#define MVN_E_PRIORS (-3)    /* Bp < 1 or B % Bp != 0 */
#define MVN_E_NULL (-4)      /* required pointer is NULL */
#define MVN_E_WORKSPACE (-5) /* workspace too small for one block */
#define MVN_E_DEVICE (-6)    /* current device is not gfx950 */

#define MVN_E_BARRIER (-7)   /* (status words only) a training launch abandoned its device-wide barrier */

#define MVN_ABI_VERSION 6 /* (6, added without a bump: mvn_vnet_byword_step_path_f32, mvn_va_byword_step_path_f32, the list steps, mvn_vnet_byword_step_states_f32, mvn_vnet_byword_step_max_symbols, mvn_vnet_byword_step_states_list_f32, mvn_vnet_byword_step_list_max_symbols, mvn_va_byword_step_states_f32, mvn_va_byword_step_states_path_f32, mvn_va_byword_step_states_list_f32, mvn_va_byword_step_max_symbols, mvn_va_byword_step_list_max_symbols, the four mvn_{vnet,va}_byword_step_256[_path]_f32 with their _max_symbols and _segment) 6: workspace arguments on mvn_vnet_decode_count_f32 (the dealt 16-state kernel's hand-off lines), + the survivor / traceback entry points (incl. mvn_vnet_decode_surv_f32) and mvn_va_montecarlo_f32; 5: + mvn_vnet_train_kernel_name, mvn_va_byword_step_f32; 4: + trial-batched training / by-word step, status words; 3: training with a workspace; 2: kernel-name queries */

/* ABI version of the loaded library (== MVN_ABI_VERSION). */
int mvn_version(void);

/* Static message for a return code of this library (never NULL). */
const char *mvn_strerror(int code);

/* 0 if the current HIP device is a gfx950 part; fills optional outputs. Host pointers. */
int mvn_device_info(int *n_cu, int *lds_bytes_per_cu, char *arch_name, int arch_name_len);

/*
 * One ACS stage, acs_block of python_code/utils/trellis_utils.py:16-30:
 *   out[b,s] = min_j (in_prob+llrs)[b,(2s+j)%S];  argmin_j[b,s] in {0,1} (int64, first minimum wins,
 *   like torch.min(dim=2)); argmin_j may be NULL.  in_prob, llrs, out: [B,S] contiguous.
 */
int mvn_acs_block_f32(const float *in_prob, const float *llrs, float *out, int64_t *argmin_j,
                      int64_t B, int32_t S, mvn_stream_t stream);

/*
 * ACS sweep over materialised branch costs: the T-step loop
 *     dec[:,i] = argmin(in_prob,1) % 2 ; in_prob = acs_block(in_prob, cost[:,i])
 * of python_code/detectors/VA/va_detector.py:89-97 (== vnet_detector.py:53-59), with
 * acs_block = python_code/utils/trellis_utils.py:16-30 and in_prob starting at zero (:84).
 *   cost [B,T,S] contiguous; dec [B, dec_ld>=T]; final_metric [B,S] or NULL.
 */
int mvn_acs_sweep_f32(const float *cost, float *dec, int64_t dec_ld, float *final_metric,
                      int64_t B, int32_t T, int32_t S, mvn_stream_t stream);

/*
 * The ViterbiNet detector with survivors (round 5): mvn_vnet_decode_f32's decisions and final metrics -- the same bits -- plus the
 * survivor planes of its sweep (branch cost = -logit, python_code/detectors/VNET/vnet_detector.py:57; acs_block's second return value,
 * utils/trellis_utils.py:30), so that mvn_traceback_f32 yields the maximum-likelihood path through the learned branch metrics -- the
 * textbook ViterbiNet decision, where the reference decides from a running argmin.  16 states, T % 4 == 0, 8-byte-aligned surv,
 * 128-byte-aligned workspace: the fused detector itself (vnet16_dealt_kernel<false, true>: survivors out of its decision pass, no
 * logits in HBM).  Otherwise the two-kernel route: the logits of as many blocks as fit `workspace` (at least T*S*4 bytes, 16-byte
 * aligned), then the survivor sweep over them.  mvn_vnet_surv_workspace_bytes: what one pass wants (hand-off lines / B*T*S*4).
 *   surv [B, T, max(1, S/8)] as for mvn_acs_sweep_surv_f32.
 */
size_t mvn_vnet_surv_workspace_bytes(int64_t B, int32_t T, int32_t S);
int mvn_vnet_decode_surv_f32(const float *y, int64_t y_ld, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *W3, const float *b3, float *dec, int64_t dec_ld, float *final_metric, uint8_t *surv,
                             void *workspace, size_t workspace_bytes, int64_t B, int32_t T, int32_t S, mvn_stream_t stream);

/*
 * The same two sweeps WITH survivor (traceback) pointers -- optional: the reference computes them and drops them (acs_block
 * returns (values, argmin_j), python_code/utils/trellis_utils.py:30; its callers keep the values only, va_detector.py:95,
 * vnet_detector.py:57), so nothing on the parity path stores or reads them.  dec and final_metric are bit for bit those of
 * mvn_acs_sweep_f32 / mvn_va_decode_f32; in addition
 *     surv[b][t][s >> 3] bit (s & 7) = argmin_j of state s at stage t  (torch.min's index: the first minimum, the first NaN),
 *     the predecessor of state s on its surviving path being (2 s + j) % S            (trellis_utils.py:7-13)
 * i.e. max(1, S / 8) bytes per symbol, mvn_survivor_bytes(B, T, S) in all, any alignment (line-aligned rows are written as whole
 * 128-byte lines).  mvn_traceback_f32 walks them back from torch.argmin(final_metric[b]) and returns the textbook
 * maximum-likelihood path: bits [B, bits_ld >= T] fp32 {0,1}, bits[b][t] = the least-significant bit of the path's state before
 * stage t (the bit of symbol t, trellis_utils.py:33-46); states int32 [B, T] = those states, or NULL.
 */
size_t mvn_survivor_bytes(int64_t B, int32_t T, int32_t S);
int mvn_acs_sweep_surv_f32(const float *cost, float *dec, int64_t dec_ld, float *final_metric, uint8_t *surv,
                           int64_t B, int32_t T, int32_t S, mvn_stream_t stream);
int mvn_va_decode_surv_f32(const float *y, int64_t y_ld, const float *state_priors, int64_t Bp, float *dec,
                           int64_t dec_ld, float *final_metric, uint8_t *surv, int64_t B, int32_t T, int32_t S,
                           mvn_stream_t stream);
int mvn_traceback_f32(const uint8_t *surv, const float *final_metric, float *bits, int64_t bits_ld, int32_t *states,
                      int64_t B, int32_t T, int32_t S, mvn_stream_t stream);

/*
 * Introspection for profiling tools (no reference counterpart): name of the device kernel mvn_acs_sweep_f32
 * launches for these buffers and this shape on the current device: the dispatcher's own decision (same MVN_*
 * environment switches, same fall-backs for buffers that are not 16-byte aligned; `cost` / `dec` are only inspected
 * for their alignment and may be NULL = aligned).  `name` is a host pointer; returns 0, or MVN_E_STATES / MVN_E_NULL.
 */
int mvn_acs_sweep_kernel_name(const float *cost, const float *dec, int64_t dec_ld, int64_t B, int32_t T, int32_t S,
                              char *name, int32_t name_len);
/* The same for mvn_va_decode_f32 and mvn_vnet_decode_f32 (two launches are reported as "a + b"; the scratch sweep of
 * the two-launch ViterbiNet route is named for 16-byte aligned buffers). */
int mvn_va_decode_kernel_name(int64_t B, int32_t T, int32_t S, char *name, int32_t name_len);
int mvn_vnet_decode_kernel_name(int64_t B, int32_t T, int32_t S, int32_t want_logits, char *name, int32_t name_len);

/*
 * VADetector.forward(y,'val'), python_code/detectors/VA/va_detector.py:73-98, given the
 * state priors of compute_state_priors (:42-50) as a [Bp,S] table (row b uses b % Bp, the
 * `.repeat` of :64-65): branch costs (y-prior)^2/2 - log(sqrt(2*pi)) (:64-68) are computed in
 * registers, never written to HBM.   y [B, y_ld>=T].
 */
int mvn_va_decode_f32(const float *y, int64_t y_ld, const float *state_priors, int64_t Bp,
                      float *dec, int64_t dec_ld, float *final_metric, int64_t B, int32_t T,
                      int32_t S, mvn_stream_t stream);

/*
 * The ViterbiNet likelihood MLP net(y.reshape(-1,1)),
 * python_code/detectors/VNET/vnet_detector.py:27-33,49 (== meta_vnet_detector.py:26-32):
 * Linear(1,100) Sigmoid Linear(100,50) ReLU Linear(50,S).  Weights in torch layout:
 * W1[100,1] b1[100] W2[50,100] b2[50] W3[S,50] b3[S]; read at call time, never cached.
 *   y [N] contiguous; logits [N,S].
 */
int mvn_vnet_logits_f32(const float *y, const float *W1, const float *b1, const float *W2,
                        const float *b2, const float *W3, const float *b3, float *logits,
                        int64_t N, int32_t S, mvn_stream_t stream);

/* Bytes of scratch mvn_vnet_decode_f32 / mvn_vnet_decode_count_f32 want to run (B,T,S) in one pass.
 *  - Two-kernel route (S = 2; S = 256; every other S != 16 below the batch size from which the fused kernel is the faster
 *    route -- about 6 blocks per CU at 4 ... 64 states, 14 at 128; MVN_UNFUSED=1): the logits of the batch; any size that
 *    holds at least one block (T*S*4 bytes) is accepted and processed in slices.
 *  - S = 16, more than 768 blocks: the hand-off lines of the dealt kernel (vnet16_dealt_kernel: the batch's 32-symbol units
 *    shared evenly by 3 workgroups per CU, a block's 16 path metrics handed from wave to wave): one 128-byte line per ring
 *    and one for the status word, (3 x CUs + 1) x 128 B with rings of 8 waves up to (8 x 3 x CUs + 1) x 128 B with rings of
 *    one (from 8 x 3 x CUs blocks on: 768 KB at 256 CUs); 128-byte aligned, contents irrelevant before and after -- a flag
 *    counts as set only when it holds a number drawn for that launch, and a graph-captured call, whose number is frozen,
 *    clears the lines itself -- not to be shared by calls that may run concurrently.  Without it
 *    (NULL / smaller / unaligned) the one-wave-per-block kernel runs: same bits, 4 % slower at 10 000 x 1000 and up to 2 x at
 *    a thousand blocks.  Word 0 of the workspace is a status word: non-zero after the call only if a hand-off wait was
 *    abandoned (the lower-numbered workgroup it waits for did not publish within seconds; the affected decisions are NaN).
 *  - 0 when the shape is served by a fused kernel that needs none (S = 4 ... 128 from those batch sizes, any batch and
 *    S = 256 with MVN_FUSED_IP=1; S = 16 up to 768 blocks of up to 1024 symbols: the cooperative kernel). */
size_t mvn_vnet_workspace_bytes(int64_t B, int32_t T, int32_t S);

/*
 * VNETDetector.forward(y,'val'), python_code/detectors/VNET/vnet_detector.py:35-61, and
 * META_VNETDetector.forward(y,'val',var), meta_vnet_detector.py:24-45 (var = the six arrays).
 *   y [B, y_ld>=T]; dec [B, dec_ld>=T]; logits_out [B,T,S] or NULL; final_metric [B,S] or NULL;
 *   workspace: device scratch of mvn_vnet_workspace_bytes(B, T, S) bytes (may be NULL when that is 0 or -- two-kernel route --
 *   logits_out is given; S = 16: optional, see there).
 *   With logits_out the logits are materialised there (S != 16: by the two-kernel route).
 */
int mvn_vnet_decode_f32(const float *y, int64_t y_ld, const float *W1, const float *b1,
                        const float *W2, const float *b2, const float *W3, const float *b3,
                        float *dec, int64_t dec_ld, float *logits_out, float *final_metric,
                        void *workspace, size_t workspace_bytes, int64_t B, int32_t T, int32_t S,
                        mvn_stream_t stream);

/*
 * One Monte-Carlo step of Trainer.single_eval_at_point (python_code/trainers/trainer.py:232-239) in ONE
 * launch, 16 states only: VNETDetector.forward(y,'val') with calculate_error_rates folded into the kernel
 * epilogue, so decisions never travel through HBM (4 B/symbol read, nothing written).
 *   tx [B, tx_ld>=K] fp32 {0,1}: transmitted words; the first K <= T columns are compared;
 *   row_mask: uint8[B] or NULL; rows with mask 0 (pilots, trainer.py:100-102) are decoded but not counted;
 *   counters: device int64[4], += {bit_errors, bits, frame_errors, frames};
 *   dec: optional [B, dec_ld>=T] decisions output (NULL = do not store);
 *   workspace / workspace_bytes: as for mvn_vnet_decode_f32 (mvn_vnet_workspace_bytes(B, T, 16); may be NULL / 0).
 * Returns MVN_E_STATES for S != 16 (use mvn_vnet_decode_f32 + mvn_count_errors there).
 */
int mvn_vnet_decode_count_f32(const float *y, int64_t y_ld, const float *W1, const float *b1,
                              const float *W2, const float *b2, const float *W3, const float *b3,
                              const float *tx, int64_t tx_ld, int32_t K, const uint8_t *row_mask,
                              int64_t *counters, float *dec, int64_t dec_ld, void *workspace,
                              size_t workspace_bytes, int64_t B, int32_t T, int32_t S, mvn_stream_t stream);

/*
 * calculate_error_rates, python_code/utils/metrics.py:7-17, as integer counters so that
 * 1/2/4/8-GPU results are identical: counters[0..3] += {bit_errors, bits, frame_errors, frames}
 * over rows `rows[i]` (int64 device array, or NULL = rows 0..n_rows-1) and the first K columns.
 * counters: device int64[4], accumulated into (caller zeroes it).
 */
int mvn_count_errors(const float *dec, int64_t dec_ld, const float *tx, int64_t tx_ld,
                     const int64_t *rows, int64_t n_rows, int32_t K, int64_t *counters,
                     mvn_stream_t stream);

/*
 * Online (self-supervised) training of the ViterbiNet MLP on ONE word, all iterations in one launch
 * (SURVEY 8f next #3): VNETTrainer.online_training, python_code/trainers/VNET/vnet_trainer.py:49-60 ->
 * Trainer.run_train_loop, trainers/trainer.py:492-505 with CrossEntropyLoss(mean) and torch.optim.Adam
 * (amsgrad off, no weight decay), i.e. n_iter x { logits = net(y); loss = CE(logits[idx_i], labels[idx_i]);
 * backward; Adam.step }.
 *   y [T] received word; labels [T] int32 trellis states (calculate_states, trellis_utils.py:33-46);
 *   batch_idx [n_iter, M] int32 sample indices per iteration (select_batch, trainer.py:534-544), or NULL = all T
 *   samples every iteration (metavnet_trainer.py:41-50);
 *   W1..b3: parameters, updated in place; adam_m/adam_v: [P] exp_avg / exp_avg_sq in parameter order
 *   (P = 250 + 50*100 + 51*S), updated in place; step0 = Adam steps already taken;
 *   loss_out [n_iter] or NULL.  S <= 256 (64 / 128 / 256 states: one workgroup per trial, the optimizer's moments stay in
 *   global memory; 256 states -- online_train_kernel<256, false>, this call, its _ws_ form and mvn_vnet_train_words_states_f32 only --
 *   also keep W3's gradient out of LDS, in the registers that accumulate it).  fp32; agrees with torch autograd + Adam to
 *   rounding, not bitwise.
 * The trainer's other optimizers (deep_learning_setup, trainer.py:163-175) ride on the same arguments: beta1 = MVN_BETA1_RMSPROP
 * runs torch.optim.RMSprop's update (alpha = beta2, eps; square average in adam_v, adam_m untouched; torch's defaults: no
 * momentum, not centered), beta1 = MVN_BETA1_SGD torch.optim.SGD's (p -= lr g; adam_m / adam_v untouched).  The same holds for
 * the _ws_ and _trials_ forms of this call (the _trials_ form: S <= 128); the meta-learning calls below take Adam only and return MVN_E_DIMS for beta1 < 0.
 */
#define MVN_BETA1_RMSPROP (-1.0f)
#define MVN_BETA1_SGD (-2.0f)
int mvn_vnet_online_train_f32(const float *y, const int32_t *labels, int32_t T, const int32_t *batch_idx, int32_t M,
                              int32_t n_iter, float *W1, float *b1, float *W2, float *b2, float *W3, float *b3,
                              float *adam_m, float *adam_v, int64_t step0, float lr, float beta1, float beta2, float eps,
                              float *loss_out, int32_t S, mvn_stream_t stream);

/*
 * The same call spread over one workgroup per 32-sample chunk when every iteration uses the whole word (batch_idx == NULL,
 * the Meta-ViterbiNet variant, metavnet_trainer.py:41-64): `workspace` = mvn_vnet_train_workspace_bytes(S) bytes of
 * device memory, 16-byte aligned, used for the gradient exchange between the workgroups (contents irrelevant before and
 * after; must not be shared by calls that may run concurrently).  Results are bit-identical to
 * mvn_vnet_online_train_f32, which also serves every case this form does not (minibatch iterations, words of at most
 * 32 symbols or more than 1024, workspace NULL or too small, MVN_TRAIN_GROUPS=0 in the environment).  S <= 256; above 32 states
 * every call runs on the one workgroup and mvn_vnet_train_workspace_bytes is 0.
 */
size_t mvn_vnet_train_workspace_bytes(int32_t n_states);
/* status: device int32[1] or NULL.  The workgroups of this form meet at a device-wide barrier whose wait is bounded (a launch
 * that cannot become resident must not hang the device).  If a wait is abandoned the weights come back as NaN AND *status is
 * set to 1 (the caller zeroes it; it is never written otherwise): check it wherever the host next synchronises -- the
 * counterpart of the reference's NaN-loss guard, trainer.py:496-498.  Concurrent launches of this form (different streams,
 * different workspaces) are safe while their combined workgroups (one per 32-sample chunk) fit the device's CUs -- words of up
 * to 256 symbols are placed on ONE XCD each (their gradient exchange stays in its L2), the XCD taken in rotation from launch to
 * launch, so that bound is then 32 CUs per XCD: at least 4 such launches per XCD, 32 on the device; to run many words at once
 * use the *_trials_* entry points below, which put them into ONE launch. */
int mvn_vnet_online_train_ws_f32(const float *y, const int32_t *labels, int32_t T, const int32_t *batch_idx, int32_t M,
                                 int32_t n_iter, float *W1, float *b1, float *W2, float *b2, float *W3, float *b3,
                                 float *adam_m, float *adam_v, int64_t step0, float lr, float beta1, float beta2, float eps,
                                 float *loss_out, int32_t S, void *workspace, size_t workspace_bytes, int32_t *status,
                                 mvn_stream_t stream);

/*
 * Joint training of the ViterbiNet MLP in ONE launch: the inner loop of Trainer.train() (trainers/trainer.py:470-479), one
 * optimizer step per word -- mvn_vnet_online_train_f32 with a word axis, the counterpart of mvn_lstm_train_f32's.
 *   y [n_words, K or more] fp32 received words (row stride y_ld), labels int32 [n_words, K or more] trellis states (row stride
 *   labels_ld); K: the positions of a word that carry a label (with use_ecc the reference hands calc_loss the 120 message bits
 *   against a 136-symbol received word: K = 120, y_ld = 136); iteration i trains on word word_of_iter[i] (device int32 [n_iter]).
 *   batch_idx [n_iter, M] device int32 positions in [0, K) (select_batch draws from arange(K), trainer.py:534-544; a position
 *   drawn twice counts twice), or NULL / M == 0: all K positions in every iteration.
 *   W1..b3, adam_m / adam_v [P], step0, lr, beta1 (Adam, or the MVN_BETA1_RMSPROP / MVN_BETA1_SGD tags), beta2, eps, loss_out
 *   [n_iter] or NULL, S <= 128: as mvn_vnet_online_train_f32.
 * One 1024-thread workgroup (online_train_words_kernel<S or 0>: the same chunk
 * code, sums and optimizer update as online_train_kernel<S, false>); with word_of_iter[i] naming rows that hold the same word the results are bit for bit those
 * of mvn_vnet_online_train_f32 on that word.  No workspace: a whole-word iteration also runs on the one workgroup.
 * Returns, in this order, before anything is launched: MVN_E_DIMS (n_iter < 0, n_words < 1, K < 1, K above a row stride, a row
 * stride above INT32_MAX, M < 0, M > K, step0 < 0), MVN_E_STATES (S above 128 or not a power of two), MVN_OK for n_iter == 0
 * (nothing is read or written), MVN_E_NULL (y, labels, word_of_iter, a weight or a moment pointer is NULL), else the launch's
 * result.  The caller's duty: every entry of word_of_iter lies in [0, n_words) and every entry of batch_idx in [0, K) -- they are
 * not checked (the call cannot see device memory) and an entry outside is read out of bounds.
 */
int mvn_vnet_train_words_f32(const float *y, int64_t y_ld, const int32_t *labels, int64_t labels_ld, int64_t n_words, int32_t K,
                             const int32_t *word_of_iter, const int32_t *batch_idx, int32_t M, int32_t n_iter, float *W1, float *b1,
                             float *W2, float *b2, float *W3, float *b3, float *adam_m, float *adam_v, int64_t step0, float lr,
                             float beta1, float beta2, float eps, float *loss_out, int32_t S, mvn_stream_t stream);

/*
 * mvn_vnet_train_words_f32 for every state count the single-trial online kernels serve, S <= 256: the same arguments, the same
 * checks and codes in the same order (MVN_E_STATES: S above 256 or not a power of two), the same launch and bits up to 128 states;
 * at 256 states (channel memory 8) online_train_words_states256_kernel, the word-axis twin of online_train_kernel<256, false> (W3's
 * gradient in the registers that accumulate it).  A call of its own, like mvn_vnet_byword_step_states_f32 beside
 * mvn_vnet_byword_step_f32: mvn_vnet_train_words_f32 keeps answering MVN_E_STATES at 256 states, which its callers may rely on.
 * (Added without a bump of MVN_ABI_VERSION, like the by-word steps.)
 */
int mvn_vnet_train_words_states_f32(const float *y, int64_t y_ld, const int32_t *labels, int64_t labels_ld, int64_t n_words, int32_t K,
                                    const int32_t *word_of_iter, const int32_t *batch_idx, int32_t M, int32_t n_iter, float *W1,
                                    float *b1, float *W2, float *b2, float *W3, float *b3, float *adam_m, float *adam_v, int64_t step0,
                                    float lr, float beta1, float beta2, float eps, float *loss_out, int32_t S, mvn_stream_t stream);

/*
 * n_steps online meta-learning steps of Meta-ViterbiNet in ONE launch: Trainer.meta_train_loop
 * (python_code/trainers/trainer.py:425-453) with METAVNETTrainer.calc_loss (metavnet_trainer.py:41-50):
 *   inner SGD step on the support words (lr = meta_lr), query loss through the updated weights, meta-gradient w.r.t.
 *   the original weights (second_order != 0: MAML with the exact Hessian-vector product; 0: first order), one Adam step.
 *   rx_words [Nw, T] fp32 received words and labels [Nw, T] int32 trellis states (calculate_states of the buffered
 *   transmitted words); step k uses the W words support_idx[k*W .. k*W+W-1] and the word query_idx[k] (indices into
 *   the Nw words, already non-negative); weights, adam_m/adam_v [P] and step0 as in mvn_vnet_online_train_f32 (the
 *   reference has one optimizer for both loops); loss_out [n_steps] query losses or NULL.  S <= 128.
 * fp32, deterministic; agrees with torch's double backward + Adam to rounding (tolerance in the tests).
 * S = 64 and 128 (maml_train_kernel<64 | 128, false>, one workgroup): the LDS holds two parameter-sized vectors, so between
 * the two gradient passes of a step the weights wait in W1 .. b3 themselves -- while the call runs these arrays hold
 * intermediate values; no workspace is needed (mvn_vnet_train_workspace_bytes stays 0 there).
 */
int mvn_vnet_maml_train_f32(const float *rx_words, const int32_t *labels, int32_t T, const int32_t *support_idx, int32_t W,
                            const int32_t *query_idx, int32_t n_steps, float *W1, float *b1, float *W2, float *b2,
                            float *W3, float *b3, float *adam_m, float *adam_v, int64_t step0, float meta_lr,
                            int32_t second_order, float lr, float beta1, float beta2, float eps, float *loss_out, int32_t S,
                            mvn_stream_t stream);

/*
 * The same steps with one workgroup per chunk of a pass (support gradient, query gradient, Hessian-vector product):
 * `workspace` as for mvn_vnet_online_train_ws_f32 (gradient exchange + private copies of the Adam moments).  Bit-identical
 * to mvn_vnet_maml_train_f32, which also serves the cases this form does not (a pass of more than 32 chunks or of one,
 * workspace NULL or too small, MVN_TRAIN_GROUPS=0 in the environment).
 */
int mvn_vnet_maml_train_ws_f32(const float *rx_words, const int32_t *labels, int32_t T, const int32_t *support_idx, int32_t W,
                               const int32_t *query_idx, int32_t n_steps, float *W1, float *b1, float *W2, float *b2,
                               float *W3, float *b3, float *adam_m, float *adam_v, int64_t step0, float meta_lr,
                               int32_t second_order, float lr, float beta1, float beta2, float eps, float *loss_out, int32_t S,
                               void *workspace, size_t workspace_bytes, int32_t *status, mvn_stream_t stream);

/*
 * R independent trials of the two training calls above in ONE launch sequence (the evaluations with online
 * training between blocks do not shard within a trial, so the parallel axis is the (SNR x seed x method) grid the reference
 * walks serially, python_code/plotters/plotter_main.py:117-149; a trial alone occupies 1-9 of the 256 CUs).  Every trial
 * has its own weights, Adam state, word(s), draws and step count, described by one mvn_train_trial_t in a DEVICE array;
 * what is common to the launch (T, M / W, the optimizer's constants, S) is passed by value.  gridDim = (chunks, trials): a
 * trial's workgroups only ever synchronise with each other (per-trial barrier counter in the workspace), trials with n = 0
 * exit at once, and a launch never holds more workgroups than the device has CUs (more trials = more launches on `stream`).
 * Per trial the results are bit-identical to the single-trial entry points.
 * State counts: mvn_vnet_online_train_trials_f32 serves S <= 128, mvn_vnet_maml_train_trials_f32 S <= 32; the meta-learning step
 * at S = 64 and 128 has a trial-batched entry point of its own, mvn_vnet_maml_train_states_trials_f32 (below: one workgroup per
 * trial, no workspace, any number of trials in one launch, and an aliasing contract for the descriptors' weight arrays).
 */
typedef struct mvn_train_trial {
    const float *y;           /* online: the word [T]; maml: the buffered received words [Nw, T] */
    const int32_t *labels;    /* online: [T]; maml: [Nw, T] (calculate_states of the buffered label words) */
    const int32_t *idx;       /* online: batch_idx [n, M] or NULL = whole word; maml: support_idx [n, W] */
    const int32_t *query_idx; /* maml: [n]; online: unused (mvn_vnet_train_words_f32 carries word_of_iter here) */
    const float *w_in[6];     /* W1, b1, W2, b2, W3, b3 read when the trial starts (e.g. the saved detector, trainer.py:275) */
    float *w_out[6];          /* ... written when it ends (may alias w_in) */
    float *w_out2[6];         /* optional second copy of the result (all six NULL: none) */
    float *adam_m, *adam_v;   /* [P] exp_avg / exp_avg_sq, updated in place */
    float *loss_out;          /* [n] or NULL */
    int32_t *status;          /* int32[1] or NULL: set to 1 if the trial's barrier wait was abandoned (weights = NaN) */
    double b1pow, b2pow;      /* (double)beta1 ** step0, (double)beta2 ** step0: Adam steps this trial has already taken */
    int32_t n;                /* iterations (online) / meta-learning steps (maml) of this trial; 0 = skip the trial */
    int32_t reserved;
} mvn_train_trial_t;

/* Device workspace for R trials of words of T symbols (W support words for the meta-learning step); 0 when the shapes run
 * on one workgroup per trial (minibatch iterations, T <= 32) and need none. */
size_t mvn_vnet_train_trials_workspace_bytes(int32_t n_states, int32_t T, int32_t W, int32_t R);
/* M = 0: every iteration uses the whole word (idx NULL in every trial); M > 0: minibatches of M samples (idx given). */
int mvn_vnet_online_train_trials_f32(const mvn_train_trial_t *trials, int32_t R, int32_t T, int32_t M, float lr, float beta1,
                                     float beta2, float eps, int32_t S, void *workspace, size_t workspace_bytes,
                                     mvn_stream_t stream);
int mvn_vnet_maml_train_trials_f32(const mvn_train_trial_t *trials, int32_t R, int32_t T, int32_t W, float meta_lr,
                                   int32_t second_order, float lr, float beta1, float beta2, float eps, int32_t S,
                                   void *workspace, size_t workspace_bytes, mvn_stream_t stream);

/*
 * The trial axis of the meta-learning step at S = 64 and 128 (mvn_vnet_maml_train_trials_f32 serves S <= 32 and returns
 * MVN_E_STATES above): maml_train_states_trials_kernel<64 | 128>, grid (1, R), trial r = trials[r] of the DEVICE array, one
 * workgroup per trial running the very body of the one-trial call.  Per trial the results are bit-identical to
 * mvn_vnet_maml_train_ws_f32 run alone.  No workspace: this form has no barrier between workgroups, so the trials of a launch
 * never wait for each other, no residency condition applies and ANY R (up to 65535) runs in ONE launch -- R above the CU count
 * simply takes ceil(R / CUs) rounds of workgroups.  A trial with n = 0 exits at once and touches nothing.
 * The aliasing contract (the LDS holds two parameter-sized vectors, so between the two gradient passes of every step the
 * weights wait in the trial's w_out arrays, which hold intermediate values while the launch runs):
 *   - a trial's w_out, w_out2, adam_m and adam_v must not overlap any array of ANOTHER trial of the launch, nor a w_in row that
 *     another trial reads (a row shared by several trials is read-only for the whole launch);
 *   - w_in is read once, before the trial's first step, and never again: it may equal the trial's own w_out (training in place)
 *     or its own w_out2 (restart from the saved detector, which is rewritten only when the trial ends), or be a row all trials
 *     share (weights_init = 'meta_training');
 *   - w_out and w_out2 of one trial must differ (w_out2 all NULL: no second copy).
 * status is never written by this call (nothing in it can give up) and loss_out may be NULL.
 * Returns, in this order: MVN_E_DIMS (T < 1, W < 1, R < 0 or > 65535, beta1 < 0: Adam only), MVN_E_STATES (S not 64 or 128),
 * MVN_OK for R == 0, MVN_E_NULL (trials == NULL), else the launch's result.
 */
int mvn_vnet_maml_train_states_trials_f32(const mvn_train_trial_t *trials, int32_t R, int32_t T, int32_t W, float meta_lr,
                                          int32_t second_order, float lr, float beta1, float beta2, float eps, int32_t S,
                                          mvn_stream_t stream);

/*
 * Introspection for tests and profiling tools (no reference counterpart): which device kernel, in which form, a training
 * call launches for these shapes on the current device -- the launchers' own decision (MVN_TRAIN_GROUPS switch, CU count,
 * the "one workgroup per chunk and trial" / "one workgroup per trial" rule for many trials).
 *   kind: 0 = mvn_vnet_online_train_*, 1 = mvn_vnet_maml_train_* first order, 2 = second order;
 *   R: 0 = the single-trial entry points, > 0 = the *_trials_* entry points with R trials that run (n > 0);
 *   M_or_W: minibatch size M (0 = whole word) for kind 0, support words W for kinds 1, 2;
 *   workspace_bytes: what the call passes (0 = no workspace).
 * name (HOST pointer) receives e.g. "maml_train_kernel<16, true> 1x176" or "online_train_groups_kernel<16, true> 5x48 in 2
 * launches one XCD per trial" (workgroups per trial x trials per launch; "one XCD per trial": the grid that places a trial's
 * workgroups on one XCD so that their gradient exchange stays in its L2 -- MVN_TRAIN_XCD=0 keeps the (groups, trials) grid).
 * S <= 128; kind 0 with R = 0 also answers at S = 256 ("online_train_kernel<256, false> 1x1", the form mvn_vnet_online_train_f32 and
 * its _ws_ form launch; mvn_vnet_train_words_states_f32 launches its word-axis twin).
 * Returns 0, MVN_E_DIMS, MVN_E_STATES or MVN_E_NULL.
 */
int mvn_vnet_train_kernel_name(int32_t kind, int32_t R, int32_t T, int32_t M_or_W, int32_t S, size_t workspace_bytes, char *name,
                               int32_t name_len);
/* The dynamic LDS (bytes) of the single-workgroup launch of that kind (online_train_kernel / maml_train_kernel, kinds 1 and 2
 * alike) at n_states; 0 where the kind does not serve that state count (kind 0, 1, 2: up to 128 states) or for another kind.
 * The counterpart of mvn_lstm_train_lds_bytes: always within one CU's 163 840 bytes. */
size_t mvn_vnet_train_lds_bytes(int32_t kind, int32_t n_states);
/* The dynamic LDS (bytes) of the single-trial online-training kernels (online_train_kernel<SC, false> and the word axis) at every
 * state count they serve, 2 ... 256: mvn_vnet_train_lds_bytes(0, n_states) up to 128 states, 158 668 at 256 (parameters, the
 * gradient vector without dW3, a chunk's images); 0 for any other n_states.  Within one CU's 163 840 bytes. */
size_t mvn_vnet_online_train_lds_bytes(int32_t n_states);

/*
 * One block step of Trainer.eval_by_word (python_code/trainers/trainer.py:292-316 and the buffer entry of :322-324) for R
 * words in ONE launch, 16 states, Reed-Solomon outer code with nsym <= 8 parity bytes:
 *   data step (pilot = 0): dec = VNETDetector.forward(rx,'val'); msg = RS-decode(dec); nerr = bit errors of msg against tx;
 *                          enc = RS-encode(msg);
 *   pilot step (pilot = 1): enc = RS-encode(tx); nerr = 0; dec and msg are not written (the reference detects the pilot too
 *                          but never uses the result);
 *   label_word = dec if nerr > 0 else enc (what the reference pushes into its buffer), labels = its trellis states
 *   (calculate_states, utils/trellis_utils.py:33-46).
 * Word r uses the weights W1 + r * w_stride[0], b1 + r * w_stride[1], ... (w_stride: HOST int64[6], NULL = one set for all):
 * R independent trials advance one block per launch; R = 1 is the reference's sequential pattern (one launch instead of
 * detect, RS decode, count, RS encode).
 *   rx [R, rx_ld >= T]; tx [R, tx_ld >= T - 8 nsym] message bits; dec / enc / label_word [R, ld >= T] or NULL;
 *   msg [R, msg_ld >= T - 8 nsym] or NULL; labels int32 [R, lab_ld >= T] or NULL; nerr int32 [R] or NULL.
 * T a multiple of 8, T <= 1024, T / 8 > nsym.  Decisions, decoded and encoded words are bit-identical to
 * mvn_vnet_decode_f32 + mvn_rs_decode_bits_f32 + mvn_rs_encode_bits_f32.  Returns MVN_E_STATES for S != 16 and MVN_E_DIMS
 * for nsym > 8 (use the separate entry points there).
 *
 * The six block steps (this one, mvn_va_byword_step_f32 and their _path_f32 / _list_f32 forms) share one check, in this order:
 * S != 16 -> MVN_E_STATES; R < 0 or a broken shape limit -> MVN_E_DIMS; (list) a broken list limit or delta_ld < T with delta given
 * -> MVN_E_DIMS; a leading dimension too small -> MVN_E_DIMS (rx_ld and tx_ld always, those of the outputs when the output is given);
 * (VA) Bp < 1 -> MVN_E_PRIORS; R = 0 -> MVN_OK before any pointer is looked at; a required pointer NULL -> MVN_E_NULL.
 * Which pointers may be NULL:
 *   every output (dec, msg, enc, label_word, labels, nerr, delta, choice) and w_stride: always;
 *   rx, and for VA state_priors: on a pilot step (pilot != 0: nothing is detected), with every entry point;
 *   tx: with the list step's data step only (then tx_ld is not looked at), unless nerr, label_word or labels is asked for;
 *   W1 .. b3: never, not even on a pilot.
 * A pilot through a _path_f32 or _list_f32 entry point is the pilot step of this one (after the list's own limits were checked).
 */
int mvn_vnet_byword_step_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                             const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                             float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                             float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                             int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);

/*
 * mvn_vnet_byword_step_f32 for the ViterbiNet detector at S = 4, 8, 32, 64 or 128 states (S = 16 forwards to it, so a caller has
 * one call for every state count): same arguments, same outputs, one launch, a workgroup per word with the word's own weights
 * (W3 [S, 50], b3 [S]).  The waves run the word's 16-symbol tiles through mvn_vnet_logits_f32's arithmetic into an on-chip image,
 * one wavefront then runs mvn_acs_sweep_f32's recurrence on it (branch cost -logit, torch.min / torch.argmin rules, always: there
 * is no fast path to guard) and carries on with the codec; labels are calculate_states with memory length log2 S.  dec is
 * bit-identical to mvn_vnet_decode_f32, the rest to mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32.
 * (Added without a bump of MVN_ABI_VERSION, like the path steps.)
 * The image bounds the word: T <= mvn_vnet_byword_step_max_symbols(S) = min(1024, what a CU's 160 KB of LDS hold next to the W3
 * image and the codec's state, in whole bytes) -- 1024 at 4, 8, 16 and 32 states, 568 at 64, 256 at 128; 0 for a state count the
 * step does not serve.
 * The check, in the order of the steps above: S not in {4, 8, 16, 32, 64, 128} -> MVN_E_STATES; R < 0, T not a multiple of 8,
 * T / 8 <= nsym, nsym outside 1 .. 8 or T > mvn_vnet_byword_step_max_symbols(S) -> MVN_E_DIMS; a leading dimension too small ->
 * MVN_E_DIMS; R = 0 -> MVN_OK; a required pointer NULL (the rules above) -> MVN_E_NULL.
 */
int32_t mvn_vnet_byword_step_max_symbols(int32_t S);
int mvn_vnet_byword_step_states_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                    const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                    float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                    float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                    int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);

/*
 * mvn_vnet_byword_step_states_f32 on the TRACED-BACK path: mvn_vnet_byword_step_path_f32 (below) for the ViterbiNet detector at
 * S = 4, 8, 32, 64 or 128 states (S = 16 forwards to it).  Same arguments, same check and codes in the same order, same longest word
 * mvn_vnet_byword_step_max_symbols(S), same outputs, one launch.  On a data step dec is bit-identical to mvn_vnet_logits_f32 ->
 * mvn_acs_sweep_surv_f32 -> mvn_traceback_f32 (= mvn_vnet_decode_surv_f32 -> mvn_traceback_f32): survivor = torch.min's index (the
 * first minimum, the first NaN), the walk starts at torch.argmin of the final metric (a NaN counting as minimal), dec[t] = the
 * least-significant bit of the path's state before stage t; msg, nerr, enc, label_word and labels follow from that dec as in
 * mvn_vnet_byword_step_states_f32.  The survivors take the place of the logits in the on-chip image, a word per stage (states s and
 * s + S / 2 share their predecessors and so their bit), and never leave the chip.  A pilot step detects nothing: it IS
 * mvn_vnet_byword_step_states_f32's pilot step.  (Added without a bump of MVN_ABI_VERSION, like the other steps.)
 */
int mvn_vnet_byword_step_states_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                         const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                         float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                         float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                         int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);

/*
 * The same block step for the classical Viterbi detector (the reference's eval_by_word takes any detector, trainer.py:295):
 * dec = VADetector.forward(rx, 'val', snr, gamma, count) with the state priors given as in mvn_va_decode_f32 -- word r uses
 * row r % Bp of state_priors [Bp, 16] (compute_state_priors, va_detector.py:42-50, of the word's channel) -- then exactly
 * the codec, label word and trellis states of mvn_vnet_byword_step_f32; same outputs, same limits (16 states, T a multiple of
 * 8, T <= 1024, nsym <= 8).  One wavefront per word.  Decisions are bit-identical to mvn_va_decode_f32, decoded / encoded
 * words to mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32.
 */
int mvn_va_byword_step_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                           float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld, float *label_word,
                           int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R, int32_t T, int32_t nsym,
                           int32_t pilot, int32_t S, mvn_stream_t stream);

/*
 * The two block steps above with the detected word taken from the TRACED-BACK Viterbi path instead of the reference's running
 * argmin: same arguments, same validation and return codes, same outputs, one launch.  On a data step
 *   dec is bit-identical to mvn_vnet_decode_surv_f32 / mvn_va_decode_surv_f32 followed by mvn_traceback_f32 (survivor = torch.min's
 *   index, NaN when either candidate is NaN; the walk starts at torch.argmin of the final metric, a NaN counting as minimal;
 *   dec[t] = the least-significant bit of the path's state before stage t),
 *   msg, nerr, enc, label_word and labels are bit-identical to mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32 (and the label
 *   rule and calculate_states above) applied to that dec.
 * The survivors never leave the chip.  The pilot step detects nothing: it IS the pilot step of the entry points above (no dec
 * or msg, nerr = 0, enc = label_word = RS-encode(tx)).
 */
int mvn_vnet_byword_step_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                  const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                  float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                  float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                  int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_va_byword_step_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                                float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);

/*
 * The path steps above with a RELIABILITY-ORDERED LIST DECODE (a Chase-type decoder judged by the trellis's own metric), one launch.
 * (Added without a bump of MVN_ABI_VERSION, like the path steps.)  All arithmetic is fp32, every operation rounded on its own.
 * With cost[t][s] the detector's branch cost of stage t for the state s before it (Viterbi: va_detector.py:64-68; ViterbiNet:
 * -logit), successors of p being p >> 1 and (p >> 1) | 8, and alpha the forward sweep the detectors run:
 *   beta_T = 0, beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | 8])
 *   delta_t = min_{s odd}(alpha_t[s] + beta_t[s]) - min_{s even}(alpha_t[s] + beta_t[s])      (the max-log LLR; its sign is dec)
 *   rho_j   = min_{i<8} |delta_{8j+i}| for the n = T / 8 bytes, parity included; the bytes are ranked by (rho, j) ascending and
 *             U = the first list_bytes of them
 *   candidate 0 = the message the path step returns for dec; candidates 1 .. C(list_bytes, nsym) = for every nsym-subset of U, in
 *             lexicographic order of rank tuples, the codeword that agrees with dec on the other n - nsym bytes (erasure filling)
 *   M(c) = sum_t cost[t][state_t(c)], ascending t, state_t = calculate_states of the (re-)encoded candidate
 *   choice = the candidate with the smallest M, the lowest index among equals.
 * msg is the chosen candidate's message; nerr, enc, label_word (dec if nerr > 0 else enc) and labels follow from it as in the
 * steps above; dec stays the traced-back word.  delta [R, >= T] (row stride delta_ld) and choice [R] may be NULL.  tx may be NULL
 * on a data step when nerr, label_word and labels are NULL: a decoder without a genie.  The pilot step is the pilot step above
 * (delta and choice are not written).
 * Limits, checked before any pointer: S = 16 (else MVN_E_STATES); T a multiple of 8, 8 (nsym + 1) <= T <= 512 (costs and alpha
 * stay in LDS, 128 B per symbol: at T = 1024 they would need 128 KB next to the ViterbiNet workgroup's 57.6 KB of weights, tiles
 * and step state, more than a CU's 160 KB); 1 <= nsym <= 8; nsym <= list_bytes <= T / 8; C(list_bytes, nsym) <= 63 (one candidate per lane of one wavefront); else
 * MVN_E_DIMS.
 * Non-finite costs: candidate 0 keeps the path step's rules; the call stays memory-safe and deterministic, but which candidate is
 * chosen is then unspecified.
 */
int mvn_vnet_byword_step_list_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                  const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                  float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                  float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                  int32_t T, int32_t nsym, int32_t pilot, int32_t S, int32_t list_bytes, float *delta,
                                  int64_t delta_ld, int32_t *choice, mvn_stream_t stream);
int mvn_va_byword_step_list_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                                float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                int32_t T, int32_t nsym, int32_t pilot, int32_t S, int32_t list_bytes, float *delta,
                                int64_t delta_ld, int32_t *choice, mvn_stream_t stream);

/*
 * mvn_vnet_byword_step_list_f32 for the ViterbiNet detector at S = 4, 8, 32, 64 or 128 states (S = 16 forwards to it, with its codes):
 * same arguments, same outputs, one launch, a workgroup per word with the word's own weights.  The definition is the one above with
 * 16 replaced by S, all in fp32 with every operation rounded on its own, cost[t][s] = -logit[t][s] of mvn_vnet_logits_f32:
 *   alpha_0 = 0, alpha_{t+1}[s] = min(alpha_t[2s % S] + cost[t][2s % S], alpha_t[(2s+1) % S] + cost[t][(2s+1) % S])
 *   dec     = what mvn_vnet_byword_step_states_path_f32 returns, bit for bit (torch.min's survivor, torch.argmin of the final metric)
 *   beta_T = 0, beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | S / 2])
 *   delta_t = min_{s odd}(alpha_t[s] + beta_t[s]) - min_{s even}(alpha_t[s] + beta_t[s])
 *   rho, the ranking by (rho, j), U, candidates 0 .. C(list_bytes, nsym), erasure filling and choice: as above
 *   M(c) = sum_t cost[t][state_t(c)], ascending t, state_t = calculate_states with memory length log2 S; the labels likewise.
 * (On chip the kernel keeps alpha_t[s] for s < S / 2 only -- states s and s + S / 2 share their predecessors -- and forms delta from
 * alpha_t[s] + min(beta_t[s], beta_t[s + S / 2]): rounded addition is monotone, so this is the value above bit for bit on finite
 * costs.)
 * Logits, the alpha half-image and the survivors stay in LDS, 4 S + 2 S + 4 bytes per symbol (8 above 32 states), and bound the
 * word: T <= mvn_vnet_byword_step_list_max_symbols(S) = min(512, what a CU's 160 KB hold next to the static part, in whole bytes)
 * -- 512 at 4, 8, 16 and 32 states, 352 at 64, 160 at 128; 0 for a state count the step does not serve.
 * The check, in the order of the steps above: S not in {4, 8, 16, 32, 64, 128} -> MVN_E_STATES; R < 0, T not a multiple of 8,
 * T / 8 <= nsym, nsym outside 1 .. 8, T > mvn_vnet_byword_step_list_max_symbols(S), list_bytes outside nsym .. T / 8,
 * C(list_bytes, nsym) > 63 or delta_ld < T -> MVN_E_DIMS; a leading dimension too small -> MVN_E_DIMS; R = 0 -> MVN_OK; a required
 * pointer NULL -> MVN_E_NULL (tx may be NULL on a data step when nerr, label_word and labels are NULL).
 * A pilot step is mvn_vnet_byword_step_states_f32's pilot step, after the list's own limits were checked (delta and choice are not
 * written).  mvn_vnet_byword_step_list_f32 itself keeps answering MVN_E_STATES for S != 16.
 * Non-finite costs: dec keeps the path step's rules; the launch stays memory-safe and deterministic, every rank, position, state
 * and candidate index stays in range; delta and choice are unspecified.
 * (Added without a bump of MVN_ABI_VERSION, like the other steps.)
 */
int32_t mvn_vnet_byword_step_list_max_symbols(int32_t S);
int mvn_vnet_byword_step_states_list_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                         const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                         float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                         float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                         int32_t T, int32_t nsym, int32_t pilot, int32_t S, int32_t list_bytes, float *delta,
                                         int64_t delta_ld, int32_t *choice, mvn_stream_t stream);

/*
 * The three block steps of the CLASSICAL Viterbi detector -- mvn_va_byword_step_f32, mvn_va_byword_step_path_f32 and
 * mvn_va_byword_step_list_f32 -- at S = 4, 8, 32, 64 or 128 states (S = 16 forwards to them, with their codes): same arguments, same
 * outputs, one launch, a workgroup per word.  Word r uses row r % Bp of state_priors [Bp, S].  The definitions are those of the
 * ViterbiNet steps at these state counts (mvn_vnet_byword_step_states_f32, _path_f32, _list_f32 above) with the branch cost
 *   cost[t][s] = (y[t] - prior[s])^2 * 0.5 - fp32(log(sqrt(2 pi)))          (va_detector.py:64-68, every operation rounded on its own)
 * in place of -logit[t][s]: the workgroup fills the on-chip image with them, one wavefront runs the recurrence with torch.min's and
 * torch.argmin's rules (always: no fast path, no guard launch) and carries on with the walk, the list decode and the codec; labels are
 * calculate_states with memory length log2 S.  Bit-identical on a data step:
 *   running  dec to mvn_va_decode_f32;
 *   path     dec to mvn_va_decode_surv_f32 -> mvn_traceback_f32;
 *   list     dec to the path step's, delta, choice and msg to the definition of mvn_vnet_byword_step_states_list_f32 on this cost;
 *   all      msg, nerr, enc, label_word and labels to mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32 and the label rule on them.
 * No weights share the LDS with the image, so the words may be longer than ViterbiNet's:
 *   T <= mvn_va_byword_step_max_symbols(S) (running, path) = min(1024, what a CU's 160 KB hold next to the codec's state, in whole
 *        bytes): 1024 at 4, 8, 16 and 32 states, 624 at 64, 312 at 128; 0 for a state count the steps do not serve;
 *   T <= mvn_va_byword_step_list_max_symbols(S) (list) = min(512, the same for 4 S + 2 S + 4 bytes per symbol, 8 above 32 states):
 *        512 at 4, 8, 16 and 32 states, 384 at 64, 192 at 128; 0 likewise.
 * The check, in the order of the steps above: S not in {4, 8, 16, 32, 64, 128} -> MVN_E_STATES; R < 0, T not a multiple of 8,
 * T / 8 <= nsym, nsym outside 1 .. 8 or T above the step's longest word -> MVN_E_DIMS; (list) list_bytes outside nsym .. T / 8,
 * C(list_bytes, nsym) > 63 or delta_ld < T with delta given -> MVN_E_DIMS; a leading dimension too small -> MVN_E_DIMS; Bp < 1 ->
 * MVN_E_PRIORS; R = 0 -> MVN_OK before any pointer is looked at; a required pointer NULL -> MVN_E_NULL (rx and state_priors may be
 * NULL on a pilot step; tx on the list's data step when nerr, label_word and labels are NULL).  A pilot step detects nothing: through
 * each of the three it is the running step's pilot (after the list's own limits were checked).
 * mvn_va_byword_step_f32, _path_f32 and _list_f32 themselves keep answering MVN_E_STATES for S != 16.
 * Non-finite costs: running and path dec keep torch.min's / torch.argmin's rules; the list's delta and choice are unspecified, the launch
 * stays memory-safe and deterministic.  (Added without a bump of MVN_ABI_VERSION, like the other steps.)
 */
int32_t mvn_va_byword_step_max_symbols(int32_t S);
int32_t mvn_va_byword_step_list_max_symbols(int32_t S);
int mvn_va_byword_step_states_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                                  float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                  float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                  int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_va_byword_step_states_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors,
                                       int64_t Bp, float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                       float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                       int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_va_byword_step_states_list_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors,
                                       int64_t Bp, float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                       float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                       int32_t T, int32_t nsym, int32_t pilot, int32_t S, int32_t list_bytes, float *delta,
                                       int64_t delta_ld, int32_t *choice, mvn_stream_t stream);

/*
 * The running and the path step of BOTH detectors at S = 256 states (channel memory 8), the one state count of the reference's trainer
 * that the calls above turn down.  Same arguments, same outputs and same definitions as mvn_vnet_byword_step_states_f32 /
 * mvn_vnet_byword_step_states_path_f32 and mvn_va_byword_step_states_f32 / mvn_va_byword_step_states_path_f32: one launch, a workgroup
 * per word, word r with its own weights (w_stride) or row r % Bp of state_priors [Bp, 256]; labels are calculate_states with memory
 * length 8.  Bit-identical on a data step:
 *   running  dec to mvn_vnet_decode_f32 / mvn_va_decode_f32 (the logits are mvn_vnet_logits_f32's);
 *   path     dec to mvn_vnet_logits_f32 / the costs above -> the survivor sweep -> mvn_traceback_f32;
 *   all      msg, nerr, enc, label_word and labels to mvn_rs_decode_bits_f32 / mvn_rs_encode_bits_f32 and the label rule on them.
 * A whole word [T][256] does not fit the LDS next to ViterbiNet's third layer, so the word passes through it in SEGMENTS of
 * mvn_vnet_byword_step_256_segment() = 80 / mvn_va_byword_step_256_segment() = 128 symbols: the workgroup fills a segment, one
 * wavefront sweeps it with the path metrics kept in registers, then the next segment is filled.  The path step keeps 16 bytes of
 * survivors per stage for the whole word.  So the longest word is the codec's:
 *   T <= mvn_vnet_byword_step_256_max_symbols() = mvn_va_byword_step_256_max_symbols() = 1024.
 * There is no list step at 256 states.  The check, in the order of the steps above: S != 256 -> MVN_E_STATES; R < 0, T not a multiple
 * of 8, T / 8 <= nsym, nsym outside 1 .. 8 or T > 1024 -> MVN_E_DIMS; a leading dimension too small -> MVN_E_DIMS; (VA) Bp < 1 ->
 * MVN_E_PRIORS; R = 0 -> MVN_OK before any pointer is looked at; a required pointer NULL -> MVN_E_NULL (rx and state_priors may be
 * NULL on a pilot step).  A pilot step detects nothing; the path step's pilot is the running step's.
 * mvn_{vnet,va}_byword_step_states[_path|_list]_f32 keep answering MVN_E_STATES for S = 256, and
 * mvn_{vnet,va}_byword_step[_list]_max_symbols(256) stay 0.  Non-finite logits, priors or received values: torch.min's /
 * torch.argmin's rules, as at the other state counts (always: no fast path, no guard launch).
 * (Added without a bump of MVN_ABI_VERSION, like the other steps.)
 */
int32_t mvn_vnet_byword_step_256_max_symbols(void);
int32_t mvn_va_byword_step_256_max_symbols(void);
int32_t mvn_vnet_byword_step_256_segment(void);
int32_t mvn_va_byword_step_256_segment(void);
int mvn_vnet_byword_step_256_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                 const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                 float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                 float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                 int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_vnet_byword_step_256_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *W1, const float *b1,
                                      const float *W2, const float *b2, const float *W3, const float *b3, const int64_t *w_stride,
                                      float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                      float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                      int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_va_byword_step_256_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                               float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                               float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                               int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);
int mvn_va_byword_step_256_path_f32(const float *rx, int64_t rx_ld, const float *tx, int64_t tx_ld, const float *state_priors, int64_t Bp,
                                    float *dec, int64_t dec_ld, float *msg, int64_t msg_ld, float *enc, int64_t enc_ld,
                                    float *label_word, int64_t lw_ld, int32_t *labels, int64_t lab_ld, int32_t *nerr, int64_t R,
                                    int32_t T, int32_t nsym, int32_t pilot, int32_t S, mvn_stream_t stream);

/* The MVN_* environment switches (A/B variants of the kernels) are read once per process; a caller that
 * changes them afterwards (the test-suite does) calls this to have them read again. */
void mvn_reload_switches(void);

/*
 * ISI-AWGN channel: ChannelModelDataset.transmit / ISIAWGNChannel.transmit,
 * python_code/channel/channel_dataset.py:71,87-95 + channel.py:12-35 + modulator.py:12:
 *   y[b,t] = sum_i h[b % Bh][L-1-i] * (1 - 2 c[b,t+i]) + sigma * w[b,t],   c = bits zero-padded past K,
 * evaluated in float64 and stored fp32 (channel_dataset.py:103).  sigma = (10**(snr/10))**-0.5 (channel.py:23,31).
 *   bits [B, ld_bits>=K] fp32 {0,1}; noise [B,T] standard-normal draws, float64 (noise_is_f64=1) or fp32, or NULL;
 *   h [Bh, L] float64 taps (estimate_channel rows); y [B, y_ld>=T].  T is normally K (transmission length).
 */
int mvn_isi_awgn_transmit(const float *bits, int64_t ld_bits, int32_t K, const void *noise, int32_t noise_is_f64,
                          const double *h, int64_t Bh, double sigma, float *y, int64_t y_ld, int64_t B, int32_t T,
                          int32_t L, mvn_stream_t stream);

/*
 * On-device word generator: the inner loop of ChannelModelDataset.get_snr_data for uncoded words
 * (python_code/channel/channel_dataset.py:65-83: random bits, zero padding by L, BPSK (modulator.py:12),
 * ISIAWGNChannel.transmit (channel.py:12-35)) fused in one kernel: bits ~ Bernoulli(1/2) and noise ~ N(0,1) from the
 * counter-based Philox4x32-10 generator (a pure function of (seed, word, position): same DISTRIBUTION as the
 * reference's two RandomState streams, not the same stream -- mvn_isi_awgn_transmit replays recorded draws bit for bit).
 *   tx [B, tx_ld>=T] transmitted bits as fp32 {0.,1.} (NULL: not stored); y [B, y_ld>=T] received words;
 *   h [Bh,L] float64 taps (row b % Bh for word b), sigma = 10^(-snr/20) (channel.py:23,31); L <= 16.
 * The function of (seed, b, t), b = b_lo + 2^32 b_hi the word and key = (seed low half, seed high half):
 *   bit c[b,t]   = bit (t % 128) of philox(key, counter (t / 128, b_lo, b_hi, 0)), least-significant bit of the first word first;
 *   noise z[b,t] : (x, y, z, w) = philox(key, counter (t / 4, b_lo, b_hi, 1)); for (a, b') = (x, y) [(z, w)], in float32,
 *                  u1 = 2^-31 ((a >> 1) + 0.5) in [2^-32, 1], u2 = 2^-32 b' in [0, 1], r = sqrt(-2 ln u1) <= sqrt(64 ln 2) ~ 6.67;
 *                  samples 4 (t / 4) + {0, 1} [{2, 3}] = r cos(2 pi u2), r sin(2 pi u2);
 *   y[b,t]       = fp32( sum_{k=0..L-1} h[b % Bh][L-1-k] (1 - 2 c[b,t+k]) + sigma z[b,t] ), c = 0 from T on, the sum and the
 *                  product in float64 in this order.
 * Nothing else enters: not B, not the tx / y layout, not h or sigma in z -- rows 0 .. B-1 of a call are the first rows of any larger
 * call, and mvn_vnet_montecarlo_f32 below addresses the same sequence from any word0 on.  tests/word_gen_ref.py is this
 * definition in NumPy; the bits and the float64 sum are reproduced bit for bit, z to the float32 accuracy of logf, sqrtf and the
 * hardware sine / cosine (a measured relative error of r: profiles/word_gen_exactness.txt).
 */
int mvn_generate_words_f32(float *tx, int64_t tx_ld, float *y, int64_t y_ld, const double *h, int64_t Bh, double sigma,
                           uint64_t seed, int64_t B, int32_t T, int32_t L, mvn_stream_t stream);

/*
 * One uncoded Monte-Carlo point of the classical Viterbi detector in ONE launch: the words of mvn_generate_words_f32 (same seed ->
 * the same bits and samples, bit for bit) are generated inside the detector of mvn_va_decode_f32 and the decisions compared with
 * the generated bits on the spot -- Trainer.single_eval_at_point, python_code/trainers/trainer.py:222-241 (draw words,
 * detector(rx, 'val'), calculate_error_rates) with no tx, y or decisions in memory ("fused into the decode kernel so y
 * never touches HBM").  counters[0..3] += {bit_errors, bits, frame_errors, frames} over B words of T symbols, exactly the counters
 * of mvn_generate_words_f32 -> mvn_va_decode_f32 -> mvn_count_errors(K = T).
 *   h [Bh,L] float64 taps (row b % Bh), sigma = 10^(-snr/20); state_priors [Bp,S] (row b % Bp: VADetector.compute_state_priors);
 *   S = 16 or 256 (MVN_E_STATES otherwise: run the three launches); counters: device int64[4], accumulated into.
 */
int mvn_va_montecarlo_f32(const double *h, int64_t Bh, double sigma, uint64_t seed, const float *state_priors, int64_t Bp,
                          int64_t *counters, int64_t B, int32_t T, int32_t L, int32_t S, mvn_stream_t stream);

/*
 * One uncoded Monte-Carlo point of the 16-state ViterbiNet, words generated inside the detector (vnet16_mc_kernel): the words of
 * mvn_generate_words_f32 (same seed -> the same bits and samples, bit for bit) detected by the fused detector of
 * mvn_vnet_decode_count_f32 and compared with the generated bits on the spot -- Trainer.single_eval_at_point,
 * python_code/trainers/trainer.py:222-241, with no tx, y or decisions in memory.  counters[0..3] += {bit_errors, bits, frame_errors,
 * frames}, exactly the counters of mvn_generate_words_f32 -> mvn_vnet_decode_count_f32(K = T) over the same words.
 *   Words are addressed globally: the call runs n_rounds rounds of B words, round r on words word0 + r B .. word0 + (r + 1) B - 1 of
 *   the generator's sequence (word w is row w of mvn_generate_words_f32 with any B > w), one launch per round, all enqueued on
 *   `stream` without a synchronisation.  stop_frame_errors = F > 0: a round runs only if counters[2] < F held when the round before
 *   it had completed (before the first one: with the counters as passed) -- a one-thread gate kernel between the rounds decides, so
 *   a round runs whole or not at all and the same arguments give the same integers every time.  F = 0 runs every round.
 *   (In a replayed graph the rule sees what earlier replays left in `counters`: zero them between replays for the eager call's
 *   integers; `progress` must be zeroed before every replay, e.g. by a memset captured in front of the call.)
 *   h [Bh,L] float64 taps (row w % Bh for word w), sigma = 10^(-snr/20); W1..b3: ViterbiNet's six arrays as in mvn_vnet_decode_f32;
 *   counters: device int64[4], accumulated into; progress: device int32[2] that the caller has ZEROED, {rounds that ran, gate flag},
 *   required when n_rounds > 1 or F > 0 and otherwise optional (NULL with n_rounds = 1, F = 0: exactly one launch).
 *   S = 16, L = 4 (MVN_E_STATES for any other S: run mvn_generate_words_f32 + mvn_vnet_decode_count_f32 there); T > 0.
 */
int mvn_vnet_montecarlo_f32(const double *h, int64_t Bh, double sigma, uint64_t seed, int64_t word0, const float *W1, const float *b1,
                            const float *W2, const float *b2, const float *W3, const float *b3, int64_t *counters, int32_t *progress,
                            int64_t B, int32_t n_rounds, int64_t stop_frame_errors, int32_t T, int32_t L, int32_t S, mvn_stream_t stream);

/*
 * Reed-Solomon outer code, batched over words; bits are fp32 {0,1}, 8 per GF(2^8)
 * symbol, MSB first (np.packbits).  Same code and same behaviour past the correction capacity as
 * python_code/ecc/rs_main.py: encode (:9-18) / decode (:21-37) -- prim 0x11d, generator 2, nsym parity bytes,
 * nbits/8 <= 255, nsym <= 64.
 *   decode: rx_bits [B, ld_in >= nbits] -> msg_bits [B, ld_out >= nbits - 8*nsym];
 *           status: int32[B] or NULL: 0 decoded, 1 = more errors than nsym/2 detected (uncorrected systematic
 *           part returned, rs_main.py:31-33), 2 = the reference would raise (never observed);
 *   encode: msg_bits [B, ld_in >= kbits] -> cw_bits [B, ld_out >= kbits + 8*nsym].
 */
int mvn_rs_decode_bits_f32(const float *rx_bits, int64_t ld_in, float *msg_bits, int64_t ld_out,
                           int32_t *status, int64_t B, int32_t nbits, int32_t nsym, mvn_stream_t stream);
int mvn_rs_encode_bits_f32(const float *msg_bits, int64_t ld_in, float *cw_bits, int64_t ld_out, int64_t B,
                           int32_t kbits, int32_t nsym, mvn_stream_t stream);

/*
 * LSTMDetector.forward(y,'val'), python_code/detectors/LSTM/lstm_detector.py:35-57, and MetaLSTMDetector.forward(y,'val',var),
 * detectors/META_LSTM/meta_lstm_detector.py:23-70 (var = the ten arrays): the window x_t = [y[t-3], y[t-2], y[t-1], y[t]] (-100
 * where the index is negative, :42-44), a unidirectional 2-layer LSTM (input 4, hidden 256, zero h and c per word, torch gate order
 * i, f, g, o), Linear(256, 2) at every t, and torch.argmax over its two logits (the first index on a tie, a NaN counts as the
 * maximum).  The sizes 4 / 256 / 2 layers / 2 classes are fixed.  Weights in torch layout, nn.LSTM.parameters() order then fc:
 * W_ih0 [1024,4] W_hh0 [1024,256] b_ih0 b_hh0 [1024] W_ih1 [1024,256] W_hh1 [1024,256] b_ih1 b_hh1 [1024] fc_W [2,256] fc_b [2];
 * read at call time, never cached.
 *   y [B, y_ld>=T]; dec [B, dec_ld>=T] fp32 {0,1}; logits [B,T,2] contiguous or NULL;
 *   workspace: mvn_lstm_workspace_bytes(B, T) bytes of device memory, 16-byte aligned (the weights repacked by the call; contents
 *   irrelevant before and after, not to be shared by calls that may run concurrently).
 * Arithmetic: every gate, and every logit, is one k-ordered fmaf chain (b_ih + b_hh, then W_ih . input, then W_hh . h; fc_b, then
 * fc_W . h), sigmoid / tanh on SLEEF's expf (lstm.inc states the formulas): bit-identical to tests/native/lstm_twin.c, and the
 * same bits for a word whatever B, its row, y_ld or the kernel form.  Returns MVN_E_DIMS for B < 0, T < 1 or a row stride < T,
 * MVN_OK for B = 0, MVN_E_NULL for a missing pointer (logits may be NULL), MVN_E_WORKSPACE for a small or unaligned workspace.
 * mvn_lstm_decode_kernel_name: the launches of the call for B words (one 16-word workgroup per tile; name is a host pointer).
 */
size_t mvn_lstm_workspace_bytes(int64_t B, int32_t T);
int mvn_lstm_decode_f32(const float *y, int64_t y_ld, const float *W_ih0, const float *W_hh0, const float *b_ih0, const float *b_hh0,
                        const float *W_ih1, const float *W_hh1, const float *b_ih1, const float *b_hh1, const float *fc_W,
                        const float *fc_b, float *dec, int64_t dec_ld, float *logits, void *workspace, size_t workspace_bytes, int64_t B,
                        int32_t T, mvn_stream_t stream);
int mvn_lstm_decode_kernel_name(int64_t B, int32_t T, char *name, int32_t name_len);

/* Training of the same network in one launch (lstm_train.inc): n_iter x {forward 'train' on ONE word, CrossEntropyLoss(mean) of the
 * two logits against the word's bits, backward through time, optimizer step}, the loop of LSTMTrainer.online_training
 * (trainers/LSTM/lstm_trainer.py:42-53), MetaLSTMTrainer.online_training (trainers/META_LSTM/meta_lstm_trainer.py:48-60) and the
 * inner loop of Trainer.train() (trainer.py:470-479).
 *   y [n_words, T] (row stride y_ld), bits int32 [n_words, T] in {0,1} (row stride bits_ld): iteration i trains on word
 *   word_of_iter[i] (NULL: word 0 in every iteration = online training).
 *   M > 0: the loss of iteration i is the mean over the M positions idx[i * M .. i * M + M) (select_batch, trainer.py:534-544; a
 *   position drawn twice counts twice); M == 0: over all T positions (idx is not read).
 *   The ten tensors (order and layout of mvn_lstm_decode_f32) and exp_avg / exp_avg_sq ([795138] floats, parameters() order) are
 *   updated in place; step0 = optimizer steps taken before the call.  beta1 >= 0: Adam (torch defaults, amsgrad off);
 *   beta1 = MVN_BETA1_RMSPROP: RMSprop with alpha = beta2 (exp_avg_sq is the square average, exp_avg is left alone);
 *   beta1 = MVN_BETA1_SGD: SGD (neither is touched).  loss_out [n_iter] or NULL.
 *   workspace: mvn_lstm_train_workspace_bytes(T) bytes of device memory, 16-byte aligned, private to the call while it runs.
 *   status: device int32 or NULL, set to 1 if a device-wide wait was abandoned (the weights are then NaN; MVN_E_BARRIER's text).
 * 1 <= T <= 256 (MVN_LSTM_TRAIN_MAX_T: the saved activations of all T steps share the LDS with the weight slices); the launch
 * uses 64 workgroups and returns MVN_E_DEVICE on a device with fewer CUs.  MVN_E_DIMS for T out of range, a row stride < T,
 * n_iter < 0, M < 0, M > T, n_words < 1 or step0 < 0 (checked before the pointers); MVN_OK for n_iter == 0.  Entries of idx outside
 * [0, T) and of word_of_iter outside [0, n_words) are the caller's error: they are not checked (the call cannot see device memory).  A
 * position outside [0, T) counts for nothing while the mean still divides by M -- where torch would raise, the loss and the
 * gradient come out too small by that share; a word outside [0, n_words) is read out of bounds.
 * Results are bit-reproducible: the same inputs give the same bits on every run, and n iterations in one call equal n1 + n2
 * iterations in two calls with the state carried over.
 * A call of more than 8192 iterations is issued as several launches of at most 8192 on the stream (the arrival counter of the
 * device-wide barrier is 32 bits wide); the result is that of one launch.
 * mvn_lstm_train_lds_bytes: the dynamic LDS of the launch for words of length T (0 for an unsupported T); it grows by 160 bytes
 * per step and is what sets MVN_LSTM_TRAIN_MAX_T.
 * mvn_lstm_train_kernel_name: the launch of such a call (name is a host pointer). */
#define MVN_LSTM_TRAIN_MAX_T 256
size_t mvn_lstm_train_workspace_bytes(int32_t T);
size_t mvn_lstm_train_lds_bytes(int32_t T);
int mvn_lstm_train_f32(const float *y, int64_t y_ld, const int32_t *bits, int64_t bits_ld, int64_t n_words,
                       const int32_t *word_of_iter, const int32_t *idx, int32_t M, int32_t n_iter, float *W_ih0, float *W_hh0,
                       float *b_ih0, float *b_hh0, float *W_ih1, float *W_hh1, float *b_ih1, float *b_hh1, float *fc_W, float *fc_b,
                       float *exp_avg, float *exp_avg_sq, int64_t step0, float lr, float beta1, float beta2, float eps,
                       float *loss_out, void *workspace, size_t workspace_bytes, int32_t *status, int32_t T, mvn_stream_t stream);
int mvn_lstm_train_kernel_name(int32_t T, int32_t M, char *name, int32_t name_len);

/* Online meta-learning of the same network in one launch (lstm_train.inc, the meta-learning form of the training kernel): n_steps x
 * Trainer.meta_train_loop (trainers/trainer.py:425-453) as MetaLSTMTrainer runs it from eval_by_word (:331-343), FIRST ORDER ONLY
 * (MAML=False, create_graph=False) and with ONE support word per step (window_size = 1).  Step k: forward, CrossEntropyLoss(mean) over
 * the whole word and backward through time on word support_idx[k] at the parameters theta; the fast weights
 * theta' = fl(theta - fl(meta_lr * g)); the same on word query_idx[k] at theta'; the query gradient -- torch.autograd.grad(loss_query,
 * params) with create_graph=False -- drives one optimizer step on THETA.  The second-order term (MAML=True) and several support
 * words are not built on the device: callers take torch autograd for them.
 *   rx_words [n_words, T] (row stride rx_ld), bits int32 [n_words, T] in {0,1} (row stride bits_ld); support_idx, query_idx: device
 *   int32 [n_steps], entries in [0, n_words) (not checked: the call cannot see device memory; a word outside is read out of bounds).
 *   The ten tensors, exp_avg, exp_avg_sq, step0, lr, beta1, beta2, eps, status: as mvn_lstm_train_f32 (Adam, RMSprop or SGD by the
 *   beta1 tag); step k is optimizer step step0 + k + 1.  loss_out [n_steps] or NULL: the query losses.
 *   workspace: mvn_lstm_maml_workspace_bytes(T) bytes of device memory, 16-byte aligned, private to the call while it runs: the
 *   training workspace and behind it the fast-weight image (theta' of W_hh0, W_ih1, W_hh1 and the fc layer, 3.15 MB).
 * 1 <= T <= MVN_LSTM_TRAIN_MAX_T; 64 workgroups, MVN_E_DEVICE on a device with fewer CUs.  MVN_E_DIMS for T out of range, a row stride
 * < T, n_steps < 0, n_words < 1 or step0 < 0 (checked before the pointers); MVN_OK for n_steps == 0; MVN_E_NULL for a missing pointer
 * (loss_out and status may be NULL); MVN_E_WORKSPACE for a small or unaligned workspace.
 * With meta_lr = 0 a step is bit for bit one whole-word iteration of mvn_lstm_train_f32 on the query word.  Results are
 * bit-reproducible and n steps in one call equal n1 + n2 steps in two.  A call of more than 4096 steps is issued as several launches
 * on the stream (two passes of the training loop per step against the 32-bit arrival counter).
 * mvn_lstm_maml_kernel_name: the launch of such a call (name is a host pointer). */
size_t mvn_lstm_maml_workspace_bytes(int32_t T);
int mvn_lstm_maml_train_f32(const float *rx_words, int64_t rx_ld, const int32_t *bits, int64_t bits_ld, int64_t n_words,
                            const int32_t *support_idx, const int32_t *query_idx, int32_t n_steps, float *W_ih0, float *W_hh0,
                            float *b_ih0, float *b_hh0, float *W_ih1, float *W_hh1, float *b_ih1, float *b_hh1, float *fc_W,
                            float *fc_b, float *exp_avg, float *exp_avg_sq, int64_t step0, float meta_lr, float lr, float beta1,
                            float beta2, float eps, float *loss_out, void *workspace, size_t workspace_bytes, int32_t *status,
                            int32_t T, mvn_stream_t stream);
int mvn_lstm_maml_kernel_name(int32_t T, char *name, int32_t name_len);

/* The LSTM trial axis: R independent trials of mvn_lstm_train_f32 / mvn_lstm_maml_train_f32 in one call (lstm_train.inc:
 * lstm_train_trials_kernel, lstm_maml_trials_kernel), and R detections side by side (lstm.inc, the trial as the second grid
 * dimension).  A training launch serves P = mvn_lstm_trials_per_launch() = min(8, CUs / 64) trials with 64 workgroups each -- 4 on
 * an MI355X -- so the whole grid is resident, one workgroup per CU; the call takes the trials with n_iter > 0 in trial order, P at a
 * time on the stream, and continues a trial of more than 8192 iterations (4096 meta-learning steps) in further launches.
 * MVN_LSTM_TRIALS_PER_LAUNCH=1..8 pins P below the device's value (tests, A/B runs).  Every trial runs the code of the single-trial
 * call on its own state, so its parameters, moments and losses are bit for bit those of that call on the trial alone; trials finish
 * independently, and a trial whose device-wide wait is abandoned writes NaN over ITS parameters and sets ITS status word.
 *   trials: HOST array of R descriptors, read before the call returns.  y / bits: the trial's words [n_words, T] with the call's
 *   row strides.  Training: iteration i trains on word word_of_iter[i] (NULL: word 0) and, for M > 0, on the positions
 *   idx[i * M .. i * M + M).  Meta-learning: step k has support word idx[k] and query word word_of_iter[k].  params: the ten tensors
 *   flat in parameters() order (795138 floats), 16-byte aligned; exp_avg / exp_avg_sq [795138]; loss_out [n_iter] or NULL;
 *   workspace: mvn_lstm_train_workspace_bytes(T) resp. mvn_lstm_maml_workspace_bytes(T) bytes, 16-byte aligned; status: device
 *   int32 or NULL.  Two trials of one call must NOT share params, moments, workspace, loss_out or status (not checked: the call
 *   cannot see device memory).  A trial with n_iter == 0 is not launched and nothing of it is read or written.
 * Checked before any device call, shapes before pointers: MVN_E_DIMS for R < 0, T outside [1, MVN_LSTM_TRAIN_MAX_T], a row stride
 * < T, M < 0, M > T, or any trial with n_iter < 0, n_words < 1 or step0 < 0; MVN_OK for R == 0 or no trial with n_iter > 0;
 * MVN_E_NULL for a missing pointer of a trial with n_iter > 0 (loss_out and status may be NULL); MVN_E_WORKSPACE for a missing or
 * misaligned workspace (or misaligned params); MVN_E_DEVICE on a device with fewer than 64 CUs.
 * mvn_lstm_decode_trials_f32: y [R B, y_ld >= T], trial r's words in rows r B .. r B + B - 1; dec [R B, dec_ld >= T] and logits
 * [R B, T, 2] (or NULL) likewise; params: the stacked bank, trial r's ten tensors flat at params + r param_ld, param_ld >= 795138
 * and a multiple of 4 (795138 is 2 mod 4 and the training kernels read the matrices with 16-byte loads: a bank stacked at the
 * natural stride would misalign every odd trial); workspace: mvn_lstm_decode_trials_workspace_bytes(R, B, T) bytes, 16-byte aligned.
 * A trial's decisions and logits are bit for bit those of mvn_lstm_decode_f32 on that trial alone.
 * mvn_lstm_train_trials_kernel_name: the launches of a training (meta = 0) or meta-learning (meta = 1) trials call. */
typedef struct mvn_lstm_trial {
    const float *y;
    const int32_t *bits;
    int64_t n_words;
    const int32_t *word_of_iter;
    const int32_t *idx;
    float *params;
    float *exp_avg, *exp_avg_sq;
    float *loss_out;
    void *workspace;
    int32_t *status;
    int64_t step0;
    int32_t n_iter;
    int32_t reserved;
} mvn_lstm_trial_t;
int32_t mvn_lstm_trials_per_launch(void);
int mvn_lstm_train_trials_f32(const mvn_lstm_trial_t *trials, int32_t R, int64_t y_ld, int64_t bits_ld, int32_t M, float lr, float beta1,
                              float beta2, float eps, int32_t T, mvn_stream_t stream);
int mvn_lstm_maml_train_trials_f32(const mvn_lstm_trial_t *trials, int32_t R, int64_t rx_ld, int64_t bits_ld, float meta_lr, float lr,
                                   float beta1, float beta2, float eps, int32_t T, mvn_stream_t stream);
int mvn_lstm_train_trials_kernel_name(int32_t R, int32_t T, int32_t meta, char *name, int32_t name_len);
size_t mvn_lstm_decode_trials_workspace_bytes(int32_t R, int64_t B, int32_t T);
int mvn_lstm_decode_trials_f32(const float *y, int64_t y_ld, const float *params, int64_t param_ld, float *dec, int64_t dec_ld,
                               float *logits, void *workspace, size_t workspace_bytes, int32_t R, int64_t B, int32_t T,
                               mvn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVN_H_ */
