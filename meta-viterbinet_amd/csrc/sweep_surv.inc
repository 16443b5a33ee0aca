// sweep_surv.inc -- the trellis sweep WITH survivor (traceback) pointers, and the traceback itself (included by mvn_hip.hip after
// the generic sweep_kernel, whose state-per-lane recurrence it repeats).
//
// The reference computes the survivors and drops them: acs_block returns (values, argmin_j) (trellis_utils.py:30) and every caller
// keeps the values only (va_detector.py:95, vnet_detector.py:57), so its detectors decide from a running argmin (SURVEY quirk Q1)
// and no traceback exists on the parity path.  These entry points are the optional output BASELINE.json's north_star names:
// the same sweep -- same decisions, same final metrics, bit for bit -- that also stores argmin_j of every state and stage,
//     surv[b][t][s >> 3] bit (s & 7) = j  with  predecessor(s) = (2 s + j) % S,   torch.min's index (first minimum, first NaN),
// one bit per state: max(1, S / 8) bytes per symbol on top of the sweep's traffic (S = 16: 2 B next to 68 B).  A wave collects the
// bits of its blocks in LDS -- one __ballot per stage and 64 states -- and writes them out 128 bytes per block at a time (64 stages
// at S = 16, 4 at S = 256): whole lines where the block's survivor row is line-aligned, dwords otherwise.
// traceback_kernel walks the survivors back from the first minimal final metric (torch.argmin) and returns the textbook
// maximum-likelihood path: bits[b][t] = sigma_t & 1, sigma_t the path's state before stage t (the state whose cost cost[b][t][.] the
// path pays; its least-significant bit is symbol t's bit, trellis_utils.py:33-46).
constexpr int kSurvLine = 128;  // bytes collected per block before they are stored

template <int S, int MODE>
__global__ __launch_bounds__(64 * kSweepWaves) void sweep_surv_kernel(
    const float *__restrict__ src, int64_t src_ld, const float *__restrict__ priors, int64_t Bp, float *__restrict__ dec,
    int64_t dec_ld, float *__restrict__ final_metric, unsigned char *__restrict__ surv, int64_t B, int T) {
    using C = SweepCfg<S>;
    constexpr int LPB = C::LPB, R = C::R, G = C::G, TC = C::TC;
    constexpr int SB = S >= 8 ? S / 8 : 1;  // survivor bytes per stage
    constexpr int KS = kSurvLine / SB;      // stages per 128 bytes
    __shared__ float lds[kSweepWaves][64 * R];
    __shared__ __attribute__((aligned(16))) unsigned char sbuf[kSweepWaves][G][kSurvLine];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / LPB;
    const int sl = lane % LPB;
    const int64_t b0 = ((int64_t)blockIdx.x * kSweepWaves + wave) * G;
    const int64_t b = b0 + g;
    const bool active = b < B;
    const int64_t bc = active ? b : B - 1;
    float *row = &lds[wave][g * S];

    float m[R], pr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        m[r] = 0.0f;
        pr[r] = 0.0f;
        if (MODE == MODE_VA) pr[r] = priors[(bc % Bp) * S + sl + LPB * r];
    }
    const float *base = (MODE == MODE_VA) ? src + bc * src_ld : src + bc * (int64_t)T * S;

    // the survivor bytes of stages [t_lo, t_hi) of this wave's blocks, from the staging buffer to surv[b][t_lo ..][.]
    auto flush = [&](int t_lo, int t_hi) {
        wave_lds_fence();
        const int nbytes = (t_hi - t_lo) * SB;
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            if (b0 + gg < B) {  // wave-uniform
                unsigned char *dst = surv + ((b0 + gg) * (int64_t)T + t_lo) * SB;
                if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
                    for (int k = lane; 4 * k < nbytes; k += 64) {
                        if (4 * k + 4 <= nbytes) {
                            reinterpret_cast<unsigned *>(dst)[k] = reinterpret_cast<const unsigned *>(sbuf[wave][gg])[k];
                        } else {
                            for (int e = 4 * k; e < nbytes; ++e) dst[e] = sbuf[wave][gg][e];
                        }
                    }
                } else {
                    for (int e = lane; e < nbytes; e += 64) dst[e] = sbuf[wave][gg][e];
                }
            }
        }
        wave_lds_fence();
    };

    float mydec = 0.0f;
    int t_flushed = 0;
    for (int t0 = 0; t0 < T; t0 += TC) {
#pragma unroll 1
        for (int i = 0; i < TC; ++i) {
            const int t = t0 + i;
            if (t < T) {  // wave-uniform
                // ---- decision: argmin over states, first minimal index (torch.argmin) % 2 (as in sweep_kernel)
                float bv = m[0];
                int bi = sl;
#pragma unroll
                for (int r = 1; r < R; ++r)
                    if (m[r] < bv || (m[r] != m[r] && bv == bv)) {
                        bv = m[r];
                        bi = sl + LPB * r;
                    }
#pragma unroll
                for (int off = 1; off < LPB; off <<= 1) {
                    float ov = __shfl_xor(bv, off);
                    int oi = __shfl_xor(bi, off);
                    const bool onan = ov != ov, bnan = bv != bv;
                    bool take = onan ? (!bnan || oi < bi) : (!bnan && ((ov < bv) || (ov == bv && oi < bi)));
                    bv = take ? ov : bv;
                    bi = take ? oi : bi;
                }
                if (sl == i) mydec = (float)(bi & 1);
                // ---- ACS stage, keeping torch.min's index
                float yv = 0.0f;
                if (MODE == MODE_VA) yv = base[t];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float c = MODE == MODE_VA ? va_cost(yv, pr[r]) : base[(int64_t)t * S + sl + LPB * r];
                    row[sl + LPB * r] = MODE == MODE_NEGLOGIT ? m[r] - c : m[r] + c;  // (ViterbiNet: branch cost = -logit, vnet_detector.py:57)
                }
                wave_lds_fence();
                const int tb = (t - t_flushed) * SB;  // byte offset of this stage in the staging buffers
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int p0 = (2 * (sl + LPB * r)) % S;
                    const float2 v = *reinterpret_cast<const float2 *>(&row[p0]);
                    const bool second = !(v.y >= v.x) && v.x == v.x;  // torch.min(dim): the first minimal index, the first NaN
                    m[r] = second ? v.y : v.x;
                    const unsigned long long bal = __ballot(second);
                    if (S >= 64) {  // lanes = states 64 r .. 64 r + 63 of the wave's one block
                        if (lane == 0) *reinterpret_cast<unsigned long long *>(&sbuf[wave][0][tb + 8 * r]) = bal;
                    } else if (sl == 0) {  // bits g S .. g S + S - 1 are block g's
                        const unsigned bits = (unsigned)(bal >> (g * S)) & (S >= 32 ? 0xffffffffu : ((1u << (S & 31)) - 1u));
                        if (SB == 4) *reinterpret_cast<unsigned *>(&sbuf[wave][g][tb]) = bits;
                        else if (SB == 2) *reinterpret_cast<unsigned short *>(&sbuf[wave][g][tb]) = (unsigned short)bits;
                        else sbuf[wave][g][tb] = (unsigned char)bits;
                    }
                }
                wave_lds_fence();
                if (t + 1 - t_flushed == KS || t + 1 == T) {
                    flush(t_flushed, t + 1);
                    t_flushed = t + 1;
                }
            }
        }
        if (active && sl < TC && t0 + sl < T) dec[b * dec_ld + t0 + sl] = mydec;
    }
    if (active && final_metric) {
#pragma unroll
        for (int r = 0; r < R; ++r) final_metric[b * S + sl + LPB * r] = m[r];
    }
}

template <int MODE>
int launch_sweep_surv(const float *src, int64_t src_ld, const float *priors, int64_t Bp, float *dec, int64_t dec_ld,
                      float *final_metric, unsigned char *surv, int64_t B, int T, int S, hipStream_t st) {
    if (B == 0 || T == 0) return MVN_OK;
#define MVN_SURV_CASE(SS)                                                                                           \
    case SS: {                                                                                                      \
        constexpr int per_wg = kSweepWaves * SweepCfg<SS>::G;                                                       \
        hipLaunchKernelGGL((sweep_surv_kernel<SS, MODE>), dim3((unsigned)((B + per_wg - 1) / per_wg)), dim3(64 * kSweepWaves), \
                           0, st, src, src_ld, priors, Bp, dec, dec_ld, final_metric, surv, B, T);                  \
        break;                                                                                                      \
    }
    switch (S) {
        MVN_SURV_CASE(2)
        MVN_SURV_CASE(4)
        MVN_SURV_CASE(8)
        MVN_SURV_CASE(16)
        MVN_SURV_CASE(32)
        MVN_SURV_CASE(64)
        MVN_SURV_CASE(128)
        MVN_SURV_CASE(256)
        default:
            return MVN_E_STATES;
    }
#undef MVN_SURV_CASE
    return (int)hipGetLastError();
}

// One lane per block: sigma_T = torch.argmin(final_metric[b]); sigma_t = (2 sigma_{t+1} + surv bit) % S; bits[b][t] = sigma_t & 1.
// The survivor bytes of consecutive stages of one block are consecutive in memory: a lane reads them backwards, 16 bytes at a time
// where the row is aligned.
__global__ __launch_bounds__(64) void traceback_kernel(const unsigned char *__restrict__ surv, const float *__restrict__ final_metric,
                                                       float *__restrict__ bits, int64_t bits_ld, int32_t *__restrict__ states,
                                                       int64_t B, int T, int S) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int SB = S >= 8 ? S / 8 : 1;
    const float *fm = final_metric + b * S;
    int s = 0;
    float mv = fm[0];
    if (mv == mv) {
        for (int k = 1; k < S; ++k) {
            const float x = fm[k];
            if (!(x >= mv)) {
                mv = x;
                s = k;
                if (x != x) break;
            }
        }
    }
    const unsigned char *sb = surv + b * (int64_t)T * SB;
    for (int t = T - 1; t >= 0; --t) {
        const int j = (sb[(int64_t)t * SB + (s >> 3)] >> (s & 7)) & 1;
        s = (2 * s + j) & (S - 1);
        bits[b * bits_ld + t] = (float)(s & 1);
        if (states) states[b * (int64_t)T + t] = s;
    }
}

// The same for S <= 32 (a step's survivors are ONE word of SB = 1, 2 or 4 bytes whose address does not depend on the path): a lane
// reads its block's row backwards in 16-byte pieces, eight of them requested while the eight before are walked, and the walk itself
// is register arithmetic -- j = (word >> sigma) & 1 -- where traceback_kernel waits for a byte load per step whose address it only
// knows after the step before (10 000 x 1000 at 16 states: 0.23 ms -> see profiles/r05_time_survivors.txt).  Bits (and states) leave as
// 16-byte stores.  The launcher takes it when the rows are 16-byte aligned (T SB % 16 == 0, aligned bases, bits_ld % 4 == 0).
template <int SB>
__global__ __launch_bounds__(64) void traceback_words_kernel(const unsigned char *__restrict__ surv, const float *__restrict__ final_metric,
                                                             float *__restrict__ bits, int64_t bits_ld, int32_t *__restrict__ states,
                                                             int64_t B, int T, int S) {
    constexpr int SPP = 16 / SB;  // steps per 16-byte piece
    constexpr int PF = 8;         // pieces in flight
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float *fm = final_metric + b * S;
    int s = 0;
    float mv = fm[0];
    if (mv == mv) {
        for (int k = 1; k < S; ++k) {
            const float x = fm[k];
            if (!(x >= mv)) {
                mv = x;
                s = k;
                if (x != x) break;
            }
        }
    }
    const uint4 *row = reinterpret_cast<const uint4 *>(surv + b * (int64_t)T * SB);
    float *brow = bits + b * bits_ld;
    int32_t *srow = states ? states + b * (int64_t)T : nullptr;
    const int npieces = T / SPP;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4 cur[PF], nxt[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) cur[k] = npieces - 1 - k >= 0 ? row[npieces - 1 - k] : zero;
    for (int p = npieces - 1; p >= 0; p -= PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) nxt[k] = p - PF - k >= 0 ? row[p - PF - k] : zero;  // (requested before the walk below)
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            if (p - k >= 0) {
                const unsigned dw[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
                int sv[SPP];
#pragma unroll
                for (int e = SPP - 1; e >= 0; --e) {
                    const unsigned w = SB == 4 ? dw[e] : SB == 2 ? dw[e >> 1] >> (16 * (e & 1)) : dw[e >> 2] >> (8 * (e & 3));
                    const int j = (int)(w >> s) & 1;
                    s = (2 * s + j) & (S - 1);
                    sv[e] = s;
                }
                const int t0 = (p - k) * SPP;
#pragma unroll
                for (int e = 0; e < SPP; e += 4) {
                    *reinterpret_cast<float4 *>(brow + t0 + e) = make_float4((float)(sv[e] & 1), (float)(sv[e + 1] & 1), (float)(sv[e + 2] & 1), (float)(sv[e + 3] & 1));
                    if (srow) *reinterpret_cast<int4 *>(srow + t0 + e) = make_int4(sv[e], sv[e + 1], sv[e + 2], sv[e + 3]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PF; ++k) cur[k] = nxt[k];
    }
}

inline int launch_traceback(const unsigned char *surv, const float *final_metric, float *bits, int64_t bits_ld, int32_t *states, int64_t B,
                            int T, int S, hipStream_t st) {
    const int SB = S >= 8 ? S / 8 : 1;
    const dim3 grid((unsigned)((B + 63) / 64));
    const bool words = S <= 32 && ((int64_t)T * SB) % 16 == 0 && (reinterpret_cast<uintptr_t>(surv) % 16) == 0 && bits_ld % 4 == 0 &&
                       (reinterpret_cast<uintptr_t>(bits) % 16) == 0 && (reinterpret_cast<uintptr_t>(states) % 16) == 0;
    if (words && SB == 1) hipLaunchKernelGGL(traceback_words_kernel<1>, grid, dim3(64), 0, st, surv, final_metric, bits, bits_ld, states, B, T, S);
    else if (words && SB == 2) hipLaunchKernelGGL(traceback_words_kernel<2>, grid, dim3(64), 0, st, surv, final_metric, bits, bits_ld, states, B, T, S);
    else if (words) hipLaunchKernelGGL(traceback_words_kernel<4>, grid, dim3(64), 0, st, surv, final_metric, bits, bits_ld, states, B, T, S);
    else hipLaunchKernelGGL(traceback_kernel, grid, dim3(64), 0, st, surv, final_metric, bits, bits_ld, states, B, T, S);
    return (int)hipGetLastError();
}
