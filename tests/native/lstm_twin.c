/*
 * lstm_twin.c -- plain C twin of lstm_decode_kernel (meta-viterbinet_amd/csrc/lstm.inc): the same fmaf chains in the same k order,
 * sigmoid and tanh on mvn_oracle_expf_u10 (oracle/libmvn_oracle.so), so its logits and decisions are the kernel's bit for bit.
 * Compiled by tests/test_lstm_host.py with gcc -ffp-contract=off (every other operation rounds once, as written).
 *
 *   y [., y_ld] received words; rows: the n_rows words to run (NULL = rows 0 .. n_rows-1); T symbols each;
 *   w: the ten arrays in LSTMDetector.parameters() order (torch layout, see include/mvn.h);
 *   logits [n_rows, T, 2] and dec [n_rows, T] of those words, in the order of `rows`.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float mvn_oracle_expf_u10(float d);

#define H 256
#define G (4 * H)

static float sigm(float z) { return 1.0f / (1.0f + mvn_oracle_expf_u10(0.0f - z)); }

static float tanh_e(float x) {
    const float e = mvn_oracle_expf_u10(-2.0f * fabsf(x));
    return copysignf((1.0f - e) / (1.0f + e), x);
}

/* gates[n] = fmaf(in[k], W[n][k], gates[n]) for k ascending; WT = W transposed, [K][G] */
static void chain(float *gates, const float *in, const float *WT, int K) {
    for (int k = 0; k < K; ++k) {
        const float a = in[k];
        const float *w = WT + (size_t)k * G;
        for (int n = 0; n < G; ++n) gates[n] = fmaf(a, w[n], gates[n]);
    }
}

static void cell(const float *gates, float *c, float *h) {
    for (int u = 0; u < H; ++u) {
        const float ig = sigm(gates[u]), fg = sigm(gates[H + u]), gg = tanh_e(gates[2 * H + u]), og = sigm(gates[3 * H + u]);
        const float cn = fg * c[u] + ig * gg;
        c[u] = cn;
        h[u] = og * tanh_e(cn);
    }
}

static float *transpose(const float *W, int K) {
    float *t = (float *)malloc(sizeof(float) * (size_t)K * G);
    for (int n = 0; n < G; ++n)
        for (int k = 0; k < K; ++k) t[(size_t)k * G + n] = W[(size_t)n * K + k];
    return t;
}

int lstm_twin(const float *y, int64_t y_ld, const float *const *w, const int64_t *rows, int64_t n_rows, int32_t T, float *logits,
              float *dec) {
    float *ih0 = transpose(w[0], 4), *hh0 = transpose(w[1], H), *ih1 = transpose(w[4], H), *hh1 = transpose(w[5], H);
    float bias0[G], bias1[G];
    for (int n = 0; n < G; ++n) {
        bias0[n] = w[2][n] + w[3][n];
        bias1[n] = w[6][n] + w[7][n];
    }
    const float *fcw = w[8], *fcb = w[9];
#pragma omp parallel for schedule(dynamic)
    for (int64_t i = 0; i < n_rows; ++i) {
        const float *yr = y + (rows ? rows[i] : i) * y_ld;
        float h0[H], c0[H], h1[H], c1[H], g[G], x[4];
        memset(h0, 0, sizeof h0);
        memset(c0, 0, sizeof c0);
        memset(h1, 0, sizeof h1);
        memset(c1, 0, sizeof c1);
        for (int t = 0; t < T; ++t) {
            for (int q = 0; q < 4; ++q) x[q] = t - 3 + q >= 0 ? yr[t - 3 + q] : -100.0f;
            memcpy(g, bias0, sizeof g);
            chain(g, x, ih0, 4);
            chain(g, h0, hh0, H);
            cell(g, c0, h0);
            memcpy(g, bias1, sizeof g);
            chain(g, h0, ih1, H);
            chain(g, h1, hh1, H);
            cell(g, c1, h1);
            float l[2];
            for (int c = 0; c < 2; ++c) {
                float a = fcb[c];
                for (int k = 0; k < H; ++k) a = fmaf(h1[k], fcw[c * H + k], a);
                l[c] = a;
            }
            logits[(i * T + t) * 2] = l[0];
            logits[(i * T + t) * 2 + 1] = l[1];
            dec[i * T + t] = (l[1] > l[0] || (isnan(l[1]) && !isnan(l[0]))) ? 1.0f : 0.0f;
        }
    }
    free(ih0);
    free(hh0);
    free(ih1);
    free(hh1);
    return 0;
}
