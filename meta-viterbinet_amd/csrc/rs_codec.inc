// rs_codec.inc -- batched Reed-Solomon outer code over GF(2^8), included by mvn_hip.hip (anonymous namespace).
//
// Counterpart of python_code/ecc/ (rs_main.py:9-37 encode/decode; rs_encoder.py:7-37; rs_decoder.py:37-218;
// polynomials_manipulation.py:85-125): prim 0x11d, generator 2, first consecutive root 2^0, systematic,
// nsym parity bytes, n = K/8 + nsym <= 255, Berlekamp-Massey + exhaustive root search + Forney, including the
// reference's behaviour past the correction capacity (uncorrected systematic part, or whatever the root
// search + Forney produce when fewer roots than the locator degree are found).  Integer/byte work: bit-exact.
//
// One lane decodes one codeword (the Monte-Carlo batch is the parallel axis); words are fp32 {0,1} bit rows
// exactly as the detectors emit them, packed MSB-first on the fly (np.packbits order).  Only the syndromes
// stream over the word; everything after works on polynomials of degree <= nsym, held in registers.
constexpr int kRsThreads = 128;

struct GfTables {
    unsigned char exp[512];
    unsigned char log[256];
};

__device__ __forceinline__ int pack_byte(const float *p) {  // 8 fp32 bits -> byte, MSB first
    int v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v = (v << 1) | ((int)p[j] & 1);
    return v;
}

struct GfConst {  // init_tables (polynomials_manipulation.py:85-110), evaluated by the compiler
    unsigned int w[(512 + 256) / 4];  // GfTables as words: exp[512] then log[256]
    constexpr GfConst() : w{} {
        unsigned char e[512] = {}, l[256] = {};
        int x = 1;
        for (int i = 0; i < 255; ++i) {
            e[i] = (unsigned char)x;
            l[x] = (unsigned char)i;
            x <<= 1;
            if (x & 0x100) x ^= 0x11d;
        }
        for (int i = 255; i < 512; ++i) e[i] = e[i - 255];
        l[0] = 0;
        for (int i = 0; i < 128; ++i) w[i] = e[4 * i] | (e[4 * i + 1] << 8) | (e[4 * i + 2] << 16) | ((unsigned)e[4 * i + 3] << 24);
        for (int i = 0; i < 64; ++i) w[128 + i] = l[4 * i] | (l[4 * i + 1] << 8) | (l[4 * i + 2] << 16) | ((unsigned)l[4 * i + 3] << 24);
    }
};
__device__ const GfConst kGfConst = GfConst();

// the tables go from constant memory to LDS, one word per thread and trip (all threads of the workgroup; no barrier here)
__device__ __forceinline__ void gf_load(GfTables *t) {
    unsigned int *dst = reinterpret_cast<unsigned int *>(t);
    for (int i = threadIdx.x; i < (512 + 256) / 4; i += blockDim.x) dst[i] = kGfConst.w[i];
}

// Words of a workgroup as packed bytes in LDS: row stride 260 B = 65 dwords, so the lanes of a wave (one word each) hit 64
// different banks.  All threads pack: item = (word, byte), consecutive threads take consecutive bytes of a word (32 B of
// bits each: coalesced), so a single codeword (B = 1, the by-word evaluation) is fetched in ONE round of loads instead
// of n dependent ones by its decoding lane.
constexpr int kRsRow = 260;
__device__ __forceinline__ void rs_stage_bytes(unsigned char *bytes, const float *base, int64_t ld, int64_t b0, int64_t B, int nbytes) {
    const int words = (int)((B - b0) < kRsThreads ? (B - b0) : kRsThreads);
    for (int item = threadIdx.x; item < words * nbytes; item += blockDim.x) {
        const int w = item / nbytes, pb = item % nbytes;
        bytes[w * kRsRow + pb] = (unsigned char)pack_byte(base + (b0 + w) * ld + 8 * pb);
    }
}
__device__ __forceinline__ void rs_unstage_bits(const unsigned char *bytes, float *base, int64_t ld, int64_t b0, int64_t B, int nbytes) {
    const int words = (int)((B - b0) < kRsThreads ? (B - b0) : kRsThreads);
    for (int item = threadIdx.x; item < words * nbytes; item += blockDim.x) {
        const int w = item / nbytes, pb = item % nbytes, byte = bytes[w * kRsRow + pb];
        float *o = base + (b0 + w) * ld + 8 * pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (float)((byte >> (7 - j)) & 1);  // np.unpackbits: MSB first
    }
}
__device__ __forceinline__ int gf_mul(const GfTables *t, int x, int y) {
    return (x == 0 || y == 0) ? 0 : t->exp[t->log[x] + t->log[y]];
}
__device__ __forceinline__ int gf_inv(const GfTables *t, int x) { return t->exp[255 - t->log[x]]; }
__device__ __forceinline__ int gf_pow2(const GfTables *t, int power) {  // gf_pow(2, power) with python's %
    int e = power % 255;
    if (e < 0) e += 255;
    return t->exp[e];
}
__device__ __forceinline__ int gf_div(const GfTables *t, int x, int y) {
    return x == 0 ? 0 : t->exp[(t->log[x] + 255 - t->log[y]) % 255];
}

// rs_find_error_locator (rs_decoder.py:140-205: Berlekamp-Massey, no erasures, synd_shift = 1) for ONE codeword.
// synd[0] = 0, synd[i + 1] = msg(2^i).  Writes the locator to err_loc[0 .. el - 1] (highest degree first, possibly with
// leading zeros: `lead` of them) and returns el; errs = el - lead - 1 errors are claimed.
template <int NS>
__device__ __forceinline__ int rs_error_locator(const GfTables *gfp, const int (&synd)[NS + 1], int nsym, int (&err_loc)[NS + 2],
                                                int &lead) {
    int old_loc[NS + 3], tmp[NS + 3];
    int el = 1, ol = 1;
    err_loc[0] = 1;
    old_loc[0] = 1;
    for (int i = 0; i < nsym; ++i) {
        const int K = i + 1;
        int delta = synd[K];
        for (int j = 1; j < el; ++j) delta ^= gf_mul(gfp, err_loc[el - (j + 1)], synd[K - j]);
        old_loc[ol++] = 0;
        if (delta != 0) {
            if (ol > el) {
                for (int t = 0; t < ol; ++t) tmp[t] = gf_mul(gfp, old_loc[t], delta);
                const int inv = gf_inv(gfp, delta);
                for (int t = 0; t < el; ++t) old_loc[t] = gf_mul(gfp, err_loc[t], inv);
                const int nl = ol;
                ol = el;
                el = nl;
                for (int t = 0; t < el; ++t) err_loc[t] = tmp[t];
            }
            const int rl = el > ol ? el : ol;  // right-aligned xor (gf_poly_add)
            for (int t = 0; t < rl; ++t) tmp[t] = 0;
            for (int t = 0; t < el; ++t) tmp[t + rl - el] = err_loc[t];
            for (int t = 0; t < ol; ++t) tmp[t + rl - ol] ^= gf_mul(gfp, old_loc[t], delta);
            el = rl;
            for (int t = 0; t < el; ++t) err_loc[t] = tmp[t];
        }
    }
    lead = 0;
    while (lead < el && err_loc[lead] == 0) ++lead;
    return el;
}

// the locator at 2^i, as rs_find_errors evaluates err_loc[::-1] (rs_decoder.py:207-218): zero <=> position n - 1 - i errs
template <class Loc>
__device__ __forceinline__ int rs_locator_at(const GfTables *gfp, const Loc &err_loc, int el, int lead, int i) {
    const int x = gf_pow2(gfp, i), rl = el - lead;
    int yv = err_loc[el - 1];
    for (int t = 1; t < rl; ++t) yv = gf_mul(gfp, yv, x) ^ err_loc[el - 1 - t];
    return yv;
}

// rs_correct_errata (rs_decoder.py:83-137, Forney) for the npos error positions pos[] (in the order the root search found
// them); corrects the message bytes row[0 .. k - 1] in place.  Returns 0, or 2 where the reference would raise.
template <int NS>
__device__ __forceinline__ int rs_forney_correct(const GfTables *gfp, const int (&synd)[NS + 1], const int *pos, int npos,
                                                 unsigned char *row, int n, int nsym) {
    const int k = n - nsym;
    int mag[NS / 2 + 1], st = 0;
    int loc[NS / 2 + 2], X[NS / 2 + 1], tmp[NS + 3];
    int ll = 1;
    loc[0] = 1;
    for (int i = 0; i < npos; ++i) {
        const int a = gf_pow2(gfp, n - 1 - pos[i]);  // multiply by [a, 1]
        // new[t] = a*loc[t] ^ loc[t-1]   (gf_poly_mul, highest degree first)
        int prev = 0;
        for (int t = 0; t <= ll; ++t) {
            const int cur = t < ll ? loc[t] : 0;
            tmp[t] = gf_mul(gfp, cur, a) ^ prev;
            prev = cur;
        }
        ll += 1;
        for (int t = 0; t < ll; ++t) loc[t] = tmp[t];
        X[i] = gf_pow2(gfp, -(255 - (n - 1 - pos[i])));
    }
    // err_eval: last ll coefficients of synd[::-1] * loc (highest degree first)
    int ev[NS / 2 + 2];
    const int pl = nsym + ll;  // product length
    for (int t = 0; t < ll; ++t) {
        const int idx = pl - ll + t;  // coefficient index in the product
        int acc = 0;
        for (int bb = 0; bb < ll; ++bb) {
            const int a = idx - bb;  // index into synd[::-1], i.e. synd[nsym - a]
            if (a >= 0 && a <= nsym) acc ^= gf_mul(gfp, synd[nsym - a], loc[bb]);
        }
        ev[t] = acc;
    }
    for (int i = 0; i < npos; ++i) {
        const int Xi_inv = gf_inv(gfp, X[i]);
        int prime = 1;
        for (int jj = 0; jj < npos; ++jj)
            if (jj != i) prime = gf_mul(gfp, prime, 1 ^ gf_mul(gfp, Xi_inv, X[jj]));
        int yv = ev[0];
        for (int t = 1; t < ll; ++t) yv = gf_mul(gfp, yv, Xi_inv) ^ ev[t];
        yv = gf_mul(gfp, X[i], yv);
        if (prime == 0) {
            st = 2;  // the reference raises ValueError here (rs_decoder.py:122-123)
            mag[i] = 0;
        } else {
            mag[i] = gf_div(gfp, yv, prime);
        }
    }
    if (st == 2) return st;
    for (int i = 0; i < npos; ++i)  // corrected message bytes: rx[:k] ^ E in the LDS image
        if (pos[i] < k) row[pos[i]] ^= (unsigned char)mag[i];
    return 0;
}

// Erasure-only Forney for ONE word (the calling lane's): the nsym byte positions pos[0 .. nsym) (distinct, < n) are erased, the
// other n - nsym bytes are kept, and mag[l] is what must be xor-ed onto byte pos[l] to make the word a codeword (the code is MDS:
// exactly one such codeword exists).  With X_l = 2^(n - 1 - pos[l]) the magnitudes solve sum_l mag_l X_l^i = synd[i + 1],
// i = 0 .. nsym - 1; with Lambda(x) = prod_m (x + X_m) and Q_l(x) = Lambda(x) / (x + X_l) = sum_i q_i x^i,
//     sum_i q_i synd[i + 1] = sum_m mag_m Q_l(X_m) = mag_l Q_l(X_l),
// so each magnitude is one synthetic division, one dot product and one Horner evaluation.  Everything stays in registers (loops
// unrolled to NS, guarded by nsym).  Positions that coincide (only possible when the caller ranked NaN reliabilities) give
// Q_l(X_l) = 0; gf_div's table index stays in range and the result is then unspecified.
template <int NS>
__device__ __forceinline__ void rs_erasure_fill(const GfTables *gfp, const int (&synd)[NS + 1], const int (&pos)[NS], int n, int nsym,
                                                int (&mag)[NS]) {
    int X[NS], lam[NS + 1];  // lam[d]: coefficient of x^d
    lam[0] = 1;
#pragma unroll
    for (int d = 1; d <= NS; ++d) lam[d] = 0;
#pragma unroll
    for (int m = 0; m < NS; ++m) {
        X[m] = m < nsym ? gf_pow2(gfp, n - 1 - pos[m]) : 0;
        if (m < nsym) {
#pragma unroll
            for (int d = NS; d >= 0; --d) lam[d] = (d > 0 ? lam[d - 1] : 0) ^ gf_mul(gfp, X[m], lam[d]);  // times (x + X_m)
        }
    }
#pragma unroll
    for (int l = 0; l < NS; ++l) {
        int q = 0, num = 0, den = 0;
#pragma unroll
        for (int d = NS; d >= 1; --d)
            if (d <= nsym) {
                q = lam[d] ^ gf_mul(gfp, X[l], q);  // q_{d-1}
                num ^= gf_mul(gfp, q, synd[d]);
                den = gf_mul(gfp, den, X[l]) ^ q;
            }
        mag[l] = l < nsym ? gf_div(gfp, num, den) : 0;
    }
}

// Everything after the syndromes for ONE codeword (the calling lane's): Berlekamp-Massey, exhaustive root search, Forney, and the
// correction of the message bytes row[0 .. n - nsym - 1] in place.  synd[0] = 0, synd[i + 1] = msg(2^i); `any` = OR of the
// syndromes.  Returns the status word of mvn_rs_decode_bits_f32 (0 decoded, 1 too many errors, 2 the reference would raise).
template <int NS>
__device__ __forceinline__ int rs_locate_correct(const GfTables &gf_, const int (&synd)[NS + 1], int any, unsigned char *row,
                                                 int n, int nsym) {
    const GfTables *const gfp = &gf_;
    if (!any) return 0;
    int err_loc[NS + 2], lead;
    const int el = rs_error_locator<NS>(gfp, synd, nsym, err_loc, lead);
    if ((el - lead - 1) * 2 > nsym) return 1;  // "too many errors": the reference returns the uncorrected systematic part (rs_main.py:31-33)
    int npos = 0, pos[NS / 2 + 1];
    for (int i = 0; i < n && npos <= NS / 2; ++i)  // roots at 2^i -> position n - 1 - i
        if (rs_locator_at(gfp, err_loc, el, lead, i) == 0) pos[npos++] = n - 1 - i;
    return rs_forney_correct<NS>(gfp, synd, pos, npos, row, n, nsym);
}

// NS = compile-time bound on nsym (polynomial storage); nsym <= NS at run time.
template <int NS>
__global__ __launch_bounds__(kRsThreads) void rs_decode_kernel(const float *__restrict__ rx, int64_t ld_in,
                                                               float *__restrict__ out, int64_t ld_out,
                                                               int *__restrict__ status, int64_t B, int n, int nsym) {
    __shared__ GfTables gf;
    __shared__ unsigned char bytes[kRsThreads * kRsRow];
    const int64_t b0 = (int64_t)blockIdx.x * blockDim.x;
    gf_load(&gf);
    rs_stage_bytes(bytes, rx, ld_in, b0, B, n);
    __syncthreads();
    const int64_t b = b0 + threadIdx.x;
    const bool live = b < B;  // (every thread stays for the barriers and the cooperative write-back)
    unsigned char *row = bytes + threadIdx.x * kRsRow;
    const int k = n - nsym;

    // rs_calc_syndromes (rs_decoder.py:37-47): synd[0] = 0, synd[i+1] = msg(2^i) by Horner, all i in one pass
    int synd[NS + 1], alpha[NS];
    synd[0] = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        synd[i + 1] = 0;
        alpha[i] = i < nsym ? gf_pow2(&gf, i) : 0;
    }
    int any = 0;
    for (int p = 0; live && p < n; ++p) {
        const int byte = row[p];
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < nsym) synd[i + 1] = gf_mul(&gf, synd[i + 1], alpha[i]) ^ byte;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) any |= synd[i + 1];

    const int st = rs_locate_correct<NS>(gf, synd, any, row, n, nsym);
    if (live && status) status[b] = st;
    __syncthreads();  // then unpacked MSB-first (np.unpackbits) by all threads
    rs_unstage_bits(bytes, out, ld_out, b0, B, k);
}

// rs_generator_poly (polynomials_manipulation.py:8-13): gen[0 .. nsym], by one thread
template <int NS>
__device__ __forceinline__ void rs_generator_poly(const GfTables &gf_, int *gen, int nsym) {
    const GfTables *const gfp = &gf_;
    int g[NS + 1], t2[NS + 2], gl = 1;
    g[0] = 1;
    for (int i = 0; i < nsym; ++i) {
        const int a = gf_pow2(gfp, i);
        int prev = 0;
        for (int t = 0; t <= gl; ++t) {  // multiply by [1, a]
            const int cur = t < gl ? g[t] : 0;
            t2[t] = cur ^ gf_mul(gfp, prev, a);
            prev = cur;
        }
        gl += 1;
        for (int t = 0; t < gl; ++t) g[t] = t2[t];
    }
    for (int t = 0; t <= nsym; ++t) gen[t] = g[t];
}

// Systematic encoding of ONE word (the calling lane's): synthetic division (rs_encoder.py:19-29) of the k message bytes
// row[0 .. k - 1] with an nsym-byte remainder register; codeword = message | remainder, written to row[k .. k + nsym - 1].
template <int NS>
__device__ __forceinline__ void rs_append_parity(const GfTables &gf_, const int *gen, unsigned char *row, int k, int nsym) {
    const GfTables *const gfp = &gf_;
    int rem[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) rem[i] = 0;
    for (int p = 0; p < k; ++p) {
        const int byte = row[p];
        const int coef = byte ^ rem[0];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int nxt = i + 1 < NS ? rem[i + 1] : 0;
            rem[i] = i < nsym ? (nxt ^ (coef ? gf_mul(gfp, gen[i + 1], coef) : 0)) : 0;
        }
        // entries at index >= nsym stay 0, so rem[nsym-1]'s "next" is 0 as required
    }
    for (int i = 0; i < nsym; ++i) row[k + i] = (unsigned char)rem[i];
}

template <int NS>
__global__ __launch_bounds__(kRsThreads) void rs_encode_kernel(const float *__restrict__ msg, int64_t ld_in,
                                                               float *__restrict__ out, int64_t ld_out, int64_t B, int k,
                                                               int nsym) {
    __shared__ GfTables gf;
    __shared__ int gen[NS + 1];
    __shared__ unsigned char bytes[kRsThreads * kRsRow];
    const int64_t b0 = (int64_t)blockIdx.x * blockDim.x;
    gf_load(&gf);
    rs_stage_bytes(bytes, msg, ld_in, b0, B, k);
    __syncthreads();
    if (threadIdx.x == 0) rs_generator_poly<NS>(gf, gen, nsym);
    __syncthreads();
    const int64_t b = b0 + threadIdx.x;
    const bool live = b < B;
    unsigned char *row = bytes + threadIdx.x * kRsRow;
    if (live) rs_append_parity<NS>(gf, gen, row, k, nsym);
    __syncthreads();
    rs_unstage_bits(bytes, out, ld_out, b0, B, k + nsym);
}
