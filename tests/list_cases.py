"""CPU referee of the by-word step with the reliability-ordered list decode (mvn_vnet_byword_step_list_f32 /
mvn_va_byword_step_list_f32), NumPy over the C oracle.  Imported by test_list_step_host.py and test_gpu_list_step.py.

  soft(cost)                     alpha [R, T + 1, 16], beta [R, T + 1, 16], delta [R, T] of the branch costs [R, T, 16], every operation
                                 an np.float32 one:  alpha_{t+1}[s] = min over p in {2s % 16, (2s + 1) % 16} of alpha_t[p] + cost[t][p],
                                 beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | 8]),
                                 delta_t = min_{s odd}(alpha_t + beta_t) - min_{s even}(alpha_t + beta_t).
  erasure_fill(bits, pos, nsym)  the codeword that agrees with the word `bits` outside the nsym bytes `pos`, by Gaussian elimination
                                 over GF(2) on the parity checks read off the generator matrix oracle.rs_encode_bits(eye(K), nsym) =
                                 [I | P]: no syndromes, no locator, no Forney.
  expected(kind, y, msg, ...)    the whole step: dec, delta, order, candidates, metrics, choice and codec_cases.reference_step on the
                                 chosen codeword (label word = dec where the chosen message has bit errors).
"""
import functools
import itertools

import numpy as np

import codec_cases as C
import oracle
import path_cases as P

f32 = np.float32


def soft(cost):
    cost = np.ascontiguousarray(cost, dtype=f32)
    R, T, S = cost.shape
    assert S == 16
    s = np.arange(S)
    p0, p1 = (2 * s) % S, (2 * s + 1) % S
    n0, n1 = s >> 1, (s >> 1) | 8
    alpha = np.zeros((R, T + 1, S), f32)
    for t in range(T):
        a = alpha[:, t] + cost[:, t]
        assert a.dtype == f32
        alpha[:, t + 1] = np.minimum(a[:, p0], a[:, p1])
    beta = np.zeros((R, T + 1, S), f32)
    for t in range(T - 1, -1, -1):
        beta[:, t] = cost[:, t] + np.minimum(beta[:, t + 1][:, n0], beta[:, t + 1][:, n1])
    ab = alpha[:, :T] + beta[:, :T]
    delta = ab[:, :, 1::2].min(axis=2) - ab[:, :, 0::2].min(axis=2)
    assert ab.dtype == f32 and delta.dtype == f32
    return alpha, beta, delta


@functools.lru_cache(maxsize=None)
def parity_checks(K, nsym):
    """H [8 nsym, K + 8 nsym] over GF(2) with H c = 0 for every codeword: [P^T | I] of the systematic generator matrix [I | P]."""
    G = oracle.rs_encode_bits(np.eye(K, dtype=f32), nsym).astype(np.uint8)
    assert np.array_equal(G[:, :K], np.eye(K, dtype=np.uint8))
    return np.concatenate([G[:, K:].T, np.eye(8 * nsym, dtype=np.uint8)], axis=1)


def _solve_gf2(A, b):
    """x with A x = b over GF(2), A square and regular."""
    n = A.shape[0]
    M = np.concatenate([A, b.reshape(-1, 1)], axis=1).astype(np.uint8)
    for col in range(n):
        piv = col + int(np.argmax(M[col:, col]))
        assert M[piv, col] == 1, "singular: the erased bytes do not determine a codeword"
        if piv != col:
            M[[col, piv]] = M[[piv, col]]
        rows = np.flatnonzero(M[:, col])
        rows = rows[rows != col]
        M[rows] ^= M[col]
    return M[:, n]


def erasure_fill(bits, byte_positions, nsym):
    bits = np.asarray(bits).astype(np.uint8)
    T = bits.shape[0]
    H = parity_checks(T - 8 * nsym, nsym)
    cols = np.concatenate([np.arange(8 * p, 8 * p + 8) for p in byte_positions])
    assert len(set(cols.tolist())) == 8 * nsym
    w0 = bits.copy()
    w0[cols] = 0
    x = _solve_gf2(H[:, cols], (H @ w0) % 2)
    w0[cols] = x
    return w0.astype(f32)


def metrics(cost, words):
    """M [R, C] = sum_t cost[r, t, state_t(words[r, c])], fp32, ascending t; words [R, C, T]."""
    R, Cn, T = words.shape
    st = oracle.calculate_states(C.L, words.reshape(R * Cn, T).astype(f32)).reshape(R, Cn, T).astype(np.int64)
    M = np.zeros((R, Cn), f32)
    rr = np.arange(R)[:, None]
    for t in range(T):
        M = M + cost[rr, t, st[:, :, t]]
    assert M.dtype == f32
    return M


def expected(kind, y, msg, nsym, m, weights=None, priors=None):
    cost = np.ascontiguousarray(P.costs(kind, y, weights, priors), dtype=f32)
    R, T, _ = cost.shape
    n = T // 8
    running, dec = P.detect(cost)
    _, _, delta = soft(cost)
    rho = np.abs(delta).reshape(R, n, 8).min(axis=2)
    order = np.argsort(rho, axis=1, kind="stable")  # (rho, j) ascending
    hard = oracle.rs_encode_bits(oracle.rs_decode_bits(np.ascontiguousarray(dec, dtype=f32), nsym), nsym)
    subsets = list(itertools.combinations(range(m), nsym))
    cands = np.zeros((R, 1 + len(subsets), T), f32)
    cands[:, 0] = hard
    for r in range(R):
        for c, sub in enumerate(subsets):
            cands[r, 1 + c] = erasure_fill(dec[r], order[r, list(sub)], nsym)
    M = metrics(cost, cands)
    choice = np.argmin(M, axis=1).astype(np.int32)  # the first minimum
    chosen = cands[np.arange(R), choice]
    step = C.reference_step(chosen, msg, nsym, False)
    assert np.array_equal(step["enc"], chosen)  # a codeword decodes to itself
    lw = np.where((step["nerr"] > 0)[:, None], dec, step["enc"]).astype(f32)
    labels = oracle.calculate_states(C.L, lw).reshape(lw.shape).astype(np.int32)
    return dict(dec=dec, running=running, delta=delta, order=order, candidates=cands, metrics=M, choice=choice, msg=step["msg"],
                nerr=step["nerr"], enc=step["enc"], label_word=lw, labels=labels)
