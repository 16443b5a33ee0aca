// lstm.inc -- the windowed two-layer LSTM detector of python_code/detectors/LSTM/lstm_detector.py (and its functional twin
// detectors/META_LSTM/meta_lstm_detector.py) for phase 'val': window, both layers, fc and torch.argmax in one kernel.
//
//   x_t = [y[t-3], y[t-2], y[t-1], y[t]] (-100 where the index is negative, lstm_detector.py:42-44);
//   per layer l (input x_t for l = 0, h0(t) for l = 1; h, c = 0 at the start of every word):
//     gate[n] = chain(b_ih[n] + b_hh[n]; W_ih[n][k] * in[k], k ascending; W_hh[n][k] * h[k], k ascending)  n = 0..1023
//     i, f, g, o = sigmoid(gate[u]), sigmoid(gate[256+u]), tanh(gate[512+u]), sigmoid(gate[768+u])
//     c = f * c + i * g;  h = o * tanh(c)                                    (torch gate order i, f, g, o)
//   logit[c] = chain(fc_b[c]; fc_W[c][k] * h1[k], k ascending);  bit = argmax(logit) (first index on a tie, NaN is the maximum)
// where chain(a; ...) is one f32 fmaf per product on an accumulator that starts at a.  That is what v_mfma_f32_16x16x4_f32 computes
// bitwise (k = lane >> 4 in order inside an instruction), so a plain C twin (tests/native/lstm_twin.c) reproduces the kernel bit for
// bit.  sigmoid(z) = sigmoid_from_neg(0 - z); tanh(x) = copysign((1 - e) / (1 + e), x), e = expf_u10(-2|x|): finite and exact at
// the ends (|x| = inf gives +-1), NaN in -> NaN out.
//
// lstm_decode_kernel<MT>: a workgroup of 16 waves owns BW = 16 * MT words (MT M-tiles of the 16x16x4 MFMA).  Wave w owns hidden
// units 16w .. 16w+15 in all four gates (N-tiles at columns u, 256+u, 512+u, 768+u), so i, f, g, o of a (word, unit) land in the
// same lane and register: the cell update runs in registers and c never leaves them.  Only h goes through LDS, double-buffered per
// layer (one barrier per layer and step), in the A-fragment order the next products read with one ds_read_b128 per 4 k-steps.
// The weights (3.2 MB) do not fit in LDS: lstm_pack_kernel writes them once per call into the caller's workspace in B-fragment
// order (one global_load_dwordx4 per lane covers 4 k-steps of one gate tile), and every step streams them from L2; the four waves
// of a SIMD cover each other's load latency (a register prefetch of the next k-group spills at the 128-VGPR cap).
// fc and the decision of step t run on the first 2 * BW lanes during step t + 1's first layer (after the loop for t = T - 1).
// Both kernels take a TRIAL as the second grid dimension (mvn_lstm_decode_trials_f32): R weight sets packed side by side, workgroup
// (x, r) decoding words 16 x .. 16 x + 15 of trial r with trial r's weights.
constexpr int kLstmIn = 4, kLstmH = 256, kLstmGates = 4 * kLstmH, kLstmWaves = 16;
constexpr float kLstmPad = -100.0f;  // START_VALUE_PADDING, lstm_detector.py:10
// packed workspace, in floats: W_ih0 [wave][gate][lane]; W_hh0, W_ih1, W_hh1 [wave][k-group of 16][gate][lane][4];
// the two layers' b_ih + b_hh [layer][1024]
constexpr size_t kLstmPkIh0 = 0;
constexpr size_t kLstmPkMat = (size_t)kLstmGates * kLstmH;  // floats of one packed 1024 x 256 matrix
constexpr size_t kLstmPkHh0 = kLstmPkIh0 + (size_t)kLstmGates * kLstmIn;
constexpr size_t kLstmPkIh1 = kLstmPkHh0 + kLstmPkMat;
constexpr size_t kLstmPkHh1 = kLstmPkIh1 + kLstmPkMat;
constexpr size_t kLstmPkBias = kLstmPkHh1 + kLstmPkMat;
constexpr size_t kLstmPkFloats = kLstmPkBias + 2 * kLstmGates;

struct LstmWeights {  // torch layout, parameters() order: per layer W_ih, W_hh, b_ih, b_hh; then fc W [2, 256], b [2]
    const float *w[10];
};

__device__ __forceinline__ float lstm_tanh(float x) {
    const float e = expf_u10(-2.0f * fabsf(x));
    return copysignf((1.0f - e) / (1.0f + e), x);
}

// one thread per packed float; blockIdx.y = trial: its ten tensors lie param_ld floats behind the previous trial's, its packed
// image kLstmPkFloats behind the previous one
__global__ __launch_bounds__(256) void lstm_pack_kernel(const LstmWeights wt, int64_t param_ld, float *__restrict__ pk) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= kLstmPkFloats) return;
    const int64_t po = (int64_t)blockIdx.y * param_ld;  // this trial's offset into every tensor
    float v;
    if (e < kLstmPkHh0) {  // [wave][gate][lane] = W_ih0[256 gate + 16 wave + (lane & 15)][lane >> 4]
        const int lane = (int)(e & 63), g = (int)(e >> 6) & 3, w = (int)(e >> 8);
        v = wt.w[0][po + (256 * g + 16 * w + (lane & 15)) * kLstmIn + (lane >> 4)];
    } else if (e < kLstmPkBias) {  // [wave][kg][gate][lane][s] = W[256 gate + 16 wave + (lane & 15)][16 kg + 4 s + (lane >> 4)]
        const int m = (int)((e - kLstmPkHh0) / kLstmPkMat);
        const size_t r = (e - kLstmPkHh0) % kLstmPkMat;
        const int s = (int)(r & 3), lane = (int)(r >> 2) & 63, g = (int)(r >> 8) & 3, kg = (int)(r >> 10) & 15, w = (int)(r >> 14);
        const float *src = wt.w[m == 0 ? 1 : (m == 1 ? 4 : 5)];
        v = src[po + (256 * g + 16 * w + (lane & 15)) * kLstmH + 16 * kg + 4 * s + (lane >> 4)];
    } else {
        const int l = (int)((e - kLstmPkBias) / kLstmGates), n = (int)((e - kLstmPkBias) % kLstmGates);
        v = wt.w[4 * l + 2][po + n] + wt.w[4 * l + 3][po + n];
    }
    pk[(size_t)blockIdx.y * kLstmPkFloats + e] = v;
}

// LDS float index of h[word m][unit k] in a buffer of BW words: [k-group][k & 3][m][(k >> 2) & 3]
template <int BW>
__device__ __forceinline__ int lstm_hidx(int m, int k) { return ((((k >> 4) * 4 + (k & 3)) * BW + m) << 2) + ((k >> 2) & 3); }

// acc[g][mt] += h . W over 256 k (k ascending) for this wave's four gate tiles; pw = this wave's slice of a packed matrix
template <int MT>
__device__ __forceinline__ void lstm_matvec(f32x4 (&acc)[4][MT], const f32x4 *__restrict__ pw, const f32x4 *hb, int lane) {
    constexpr int BW = 16 * MT;
    const int j = lane & 15, q = lane >> 4;
    f32x4 bcur[4];
#pragma unroll 1
    for (int kg = 0; kg < 16; ++kg) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bcur[g] = pw[(kg * 4 + g) * 64 + lane];
        f32x4 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = hb[(kg * 4 + q) * BW + 16 * mt + j];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[g][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][s], bcur[g][s], acc[g][mt], 0, 0, 0);
    }
}

// the cell update of one layer: gates in acc (C layout: word 16 mt + 4 (lane >> 4) + r, unit 16 wave + (lane & 15)), c in
// registers, h into the LDS buffer hb
template <int MT>
__device__ __forceinline__ void lstm_cell(const f32x4 (&acc)[4][MT], float (&c)[MT][4], float *hb, int wave, int lane) {
    constexpr int BW = 16 * MT;
    const int u = 16 * wave + (lane & 15);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = sigmoid_from_neg(0.0f - acc[0][mt][r]);
            const float fg = sigmoid_from_neg(0.0f - acc[1][mt][r]);
            const float gg = lstm_tanh(acc[2][mt][r]);
            const float og = sigmoid_from_neg(0.0f - acc[3][mt][r]);
            const float cn = fg * c[mt][r] + ig * gg;
            c[mt][r] = cn;
            hb[lstm_hidx<BW>(16 * mt + 4 * (lane >> 4) + r, u)] = og * lstm_tanh(cn);
        }
}

// fc + argmax of step t for word m = tid >> 1 (class tid & 1); h1 of that step in hb
template <int BW>
__device__ __forceinline__ void lstm_fc(const float *hb, const float *fcw, float fcb, int tid, int64_t b0, int64_t B, int T, int t,
                                        float *__restrict__ dec, int64_t dec_ld, float *__restrict__ logits) {
    const int m = tid >> 1, cls = tid & 1;
    const f32x4 *hv = reinterpret_cast<const f32x4 *>(hb);
    float acc = fcb;
#pragma unroll 1
    for (int kg = 0; kg < 16; ++kg) {
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = hv[(kg * 4 + q) * BW + m];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(fcw[cls * kLstmH + 16 * kg + 4 * s + q], v[q][s], acc);
    }
    const float other = __shfl_xor(acc, 1);
    const int64_t b = b0 + m;
    if (b >= B) return;
    if (logits) logits[(b * T + t) * 2 + cls] = acc;
    if (cls == 0) {  // torch.argmax over (l0, l1): index 1 only if l1 is the first maximum (a NaN counts as the maximum)
        const bool one = (other > acc) || (other != other && acc == acc);
        dec[b * dec_ld + t] = one ? 1.0f : 0.0f;
    }
}

// TRIALS: blockIdx.y = trial (mvn_lstm_decode_trials_f32); false keeps the single-trial launch the code it was, instruction for
// instruction (the trial offsets cost the register allocation 8 VGPRs and 2.5 % of the kernel's time at 1 x 136)
template <int MT, bool TRIALS = false>
__global__ __launch_bounds__(64 * kLstmWaves) void lstm_decode_kernel(const float *__restrict__ y, int64_t y_ld,
                                                                      const float *__restrict__ pk, const float *__restrict__ fc_w,
                                                                      const float *__restrict__ fc_b, float *__restrict__ dec,
                                                                      int64_t dec_ld, float *__restrict__ logits, int64_t B, int T,
                                                                      int64_t param_ld) {
    constexpr int BW = 16 * MT;
    constexpr int HBUF = BW * kLstmH;  // floats of one h buffer
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *h0 = smem;              // [2][HBUF] layer-0 h, buffer t & 1 holds h0(t)
    float *h1 = smem + 2 * HBUF;   // [2][HBUF] layer-1 h
    float *fcw = smem + 4 * HBUF;  // [2][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    // blockIdx.y = trial r: rows r B .. r B + B - 1 of y / dec / logits (B_end = their end), its own packed weights and fc layer
    const int64_t trial = TRIALS ? blockIdx.y : 0;
    const int64_t row0 = trial * B, B_end = row0 + B, b0 = row0 + (int64_t)blockIdx.x * BW;
    const float *__restrict__ pkr = pk + trial * (int64_t)kLstmPkFloats;
    const int64_t po = trial * param_ld;

    for (int i = tid; i < HBUF; i += 64 * kLstmWaves) {  // h(-1) = 0 (buffer 1 of both layers)
        h0[HBUF + i] = 0.0f;
        h1[HBUF + i] = 0.0f;
    }
    for (int i = tid; i < 2 * kLstmH; i += 64 * kLstmWaves) fcw[i] = fc_w[po + i];
    const float fcb = tid < 2 * BW ? fc_b[po + (tid & 1)] : 0.0f;

    const int u = 16 * wave + j;  // this lane's hidden unit (C column)
    float bias0[4], bias1[4], wih0[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bias0[g] = pkr[kLstmPkBias + 256 * g + u];
        bias1[g] = pkr[kLstmPkBias + kLstmGates + 256 * g + u];
        wih0[g] = pkr[kLstmPkIh0 + (wave * 4 + g) * 64 + lane];
    }
    const float *yrow[MT];  // A fragment of x_t: word 16 mt + j, input k = q (rows past the trial's last read that one; nothing is stored for them)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int64_t b = b0 + 16 * mt + j;
        yrow[mt] = y + (b < B_end ? b : B_end - 1) * y_ld;
    }
    float xn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xn[mt] = q >= 3 ? yrow[mt][q - 3] : kLstmPad;
    float c0[MT][4], c1[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) c0[mt][r] = c1[mt][r] = 0.0f;

    const f32x4 *pk4 = reinterpret_cast<const f32x4 *>(pkr);
    const f32x4 *whh0 = pk4 + (kLstmPkHh0 + (size_t)wave * 16384) / 4;
    const f32x4 *wih1 = pk4 + (kLstmPkIh1 + (size_t)wave * 16384) / 4;
    const f32x4 *whh1 = pk4 + (kLstmPkHh1 + (size_t)wave * 16384) / 4;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1, prv = cur ^ 1;
        float xa[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            xa[mt] = xn[mt];
            const int tt = t - 2 + q;  // x_{t+1}[q] = y[t + 1 - 3 + q]
            if (t + 1 < T) xn[mt] = tt >= 0 ? yrow[mt][tt] : kLstmPad;
        }
        // layer 0
        f32x4 acc[4][MT];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[g][mt] = f32x4{bias0[g], bias0[g], bias0[g], bias0[g]};
                acc[g][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[mt], wih0[g], acc[g][mt], 0, 0, 0);
            }
        lstm_matvec<MT>(acc, whh0, reinterpret_cast<const f32x4 *>(h0 + prv * HBUF), lane);
        lstm_cell<MT>(acc, c0, h0 + cur * HBUF, wave, lane);
        if (t > 0 && tid < 2 * BW) lstm_fc<BW>(h1 + prv * HBUF, fcw, fcb, tid, b0, B_end, T, t - 1, dec, dec_ld, logits);
        __syncthreads();
        // layer 1
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[g][mt] = f32x4{bias1[g], bias1[g], bias1[g], bias1[g]};
        lstm_matvec<MT>(acc, wih1, reinterpret_cast<const f32x4 *>(h0 + cur * HBUF), lane);
        lstm_matvec<MT>(acc, whh1, reinterpret_cast<const f32x4 *>(h1 + prv * HBUF), lane);
        lstm_cell<MT>(acc, c1, h1 + cur * HBUF, wave, lane);
        __syncthreads();
    }
    if (tid < 2 * BW) lstm_fc<BW>(h1 + ((T - 1) & 1) * HBUF, fcw, fcb, tid, b0, B_end, T, T - 1, dec, dec_ld, logits);
}

constexpr size_t lstm_lds_bytes(int mt) { return ((size_t)4 * 16 * mt * kLstmH + 2 * kLstmH) * sizeof(float); }

// One form: MT = 1 (16 words per workgroup, 98 VGPRs, no scratch).  MT = 2 (each B fragment serving two M-tiles, half the L2
// traffic) needs 14 VGPRs more than the 128 a 1024-thread workgroup may hold and spills; it is not launched (DESIGN 5.9).
// R trials (grid y): trial r's tensors at wt.w[i] + r param_ld, its B words at row r B of y / dec / logits
int launch_lstm_decode(const float *y, int64_t y_ld, const LstmWeights &wt, float *dec, int64_t dec_ld, float *logits, float *pk,
                       int64_t B, int T, hipStream_t st, int R = 1, int64_t param_ld = 0) {
    hipLaunchKernelGGL(lstm_pack_kernel, dim3((unsigned)((kLstmPkFloats + 255) / 256), (unsigned)R), dim3(256), 0, st, wt, param_ld, pk);
    const dim3 grid((unsigned)((B + 15) / 16), (unsigned)R);
    const size_t lds = lstm_lds_bytes(1);
    const auto kernel = R > 1 ? lstm_decode_kernel<1, true> : lstm_decode_kernel<1, false>;
    if (int e = ensure_dynamic_lds((const void *)kernel, lds)) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(64 * kLstmWaves), lds, st, y, y_ld, (const float *)pk, wt.w[8], wt.w[9], dec,
                       dec_ld, logits, B, T, param_ld);
    return (int)hipGetLastError();
}
