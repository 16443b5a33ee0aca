"""Inputs on which the ViterbiNet kernels' data-dependent choices are reached, and plain NumPy references for them.  CPU only;
imported by test_exact_nets_host.py and test_gpu_exact_nets.py.

  staircase_weights / ideal_logits / textbook_acs / tie_case
      Networks whose logits are exact multiples of 1/4 in ANY summation order, so that path metrics tie again and again after
      symbol 0 (random real-valued weights tie at symbol 0 only), with a float64 MLP and a textbook Viterbi as the reference.
  ladder_weights / ladder_samples
      Samples that put a tile's sigmoid bound max|y| max|W1| + max|b1| on, just below and just above the fast form's limit 86,
      into the range where 1 / (1 + e) is a subnormal float, and up to the largest floats.
  subnormal_net / subnormal_samples
      A network in which one subnormal hidden-1 activation alone decides a logit.
"""
import functools

import numpy as np

H1, H2 = 100, 50
GRID_FAST = np.array([-1.0, 1.0], np.float32)
GRID_SLOW = (np.arange(-3, 3) + 0.5).astype(np.float32)  # k + 0.5, k = -3..2
W2_DENSITY, W3_DENSITY = 0.05, 0.08
STRICT_B2 = np.float32(1e15)  # > kStrictMinBound (1e14): the kernels take their NaN-propagating forms


def staircase_weights(S, rng, fast, strict=False):
    """A ViterbiNet [W1, b1, W2, b2, W3, b3] whose logits are exact multiples of 1/4 whatever the order of summation.
    Layer 1 is a step: W1 = +-a, b1 = -+a theta, so that sigmoid(W1 y + b1) is 1.0f exactly or at most e^-64 (which no sum that
    also holds b2 = integer + 0.5 can see).  fast: a = 64, theta = 0, for y in GRID_FAST (bound 64: the fast sigmoid); else
    a = 128, theta in {-2..2}, for y in GRID_SLOW (bound 576: the IEEE-division form, exp clamped both ways).  Layer 2: sparse
    integers, b2 = integer + 0.5; layer 3: sparse {-1, 0, 1}, b3 in {+-0.25, +-0.75}.  strict: one hidden-2 unit with an all-zero
    W3 column gets b2 = 1e15, which sends every kernel to its strict (torch.min) form and changes no logit."""
    sign = rng.choice([-1.0, 1.0], H1)
    a = 64.0 if fast else 128.0
    theta = np.zeros(H1) if fast else rng.randint(-2, 3, H1).astype(np.float64)
    W1 = (sign * a).reshape(H1, 1)
    b1 = -sign * a * theta + 0.0  # (+ 0.0: no -0)
    W2 = rng.choice([-2.0, -1.0, 1.0, 2.0], (H2, H1)) * (rng.rand(H2, H1) < W2_DENSITY)
    b2 = rng.randint(-2, 3, H2) + 0.5
    W3 = rng.choice([-1.0, 1.0], (S, H2)) * (rng.rand(S, H2) < W3_DENSITY)
    b3 = rng.choice([-0.75, -0.25, 0.25, 0.75], S)
    if strict:
        j = int(rng.randint(H2))
        W3[:, j] = 0.0
        b2[j] = STRICT_B2
    return [np.ascontiguousarray(x, dtype=np.float32) for x in (W1, b1, W2, b2, W3, b3)]


def ideal_logits(y, w):
    """The staircase network in float64 with layer 1 as the ideal step: [..., S]."""
    W1, b1, W2, b2, W3, b3 = [np.asarray(x, np.float64) for x in w]
    h1 = (np.asarray(y, np.float64)[..., None] * W1[:, 0] + b1 > 0).astype(np.float64)
    h2 = np.maximum(h1 @ W2.T + b2, 0.0)
    return h2 @ W3.T + b3


def textbook_acs(cost, last=False):
    """The reference's detection loop over branch costs [B, T, S], zero initial metrics: before each stage the decision
    argmin(metrics) % 2, then out[s] = min over the predecessors (2s) % S and (2s+1) % S of metric + cost (the cost indexed by the
    predecessor); the first index wins a tie, the last with last=True.  Returns decisions [B, T] f32, final metrics [B, S] f32,
    survivor bits packed uint8 [B, T, max(1, S/8)] (bit s & 7 of byte s >> 3) and the traced-back path's bits [B, T] f32."""
    cost = np.asarray(cost, np.float32)
    B, T, S = cost.shape
    rows, s_idx = np.arange(B)[:, None], np.arange(S)
    p0, p1 = (2 * s_idx) % S, (2 * s_idx + 1) % S
    argmin = (lambda m: S - 1 - np.argmin(m[:, ::-1], axis=1)) if last else (lambda m: np.argmin(m, axis=1))
    m = np.zeros((B, S), np.float32)
    dec = np.zeros((B, T), np.float32)
    take1 = np.zeros((B, T, S), bool)
    for t in range(T):
        dec[:, t] = argmin(m) % 2
        a = m + cost[:, t]
        c0, c1 = a[:, p0], a[:, p1]
        take1[:, t] = (c1 <= c0) if last else (c1 < c0)
        m = np.where(take1[:, t], c1, c0)
    bits = np.zeros((B, T, max(8, S)), np.uint8)
    bits[:, :, :S] = take1
    surv = np.packbits(bits, axis=2, bitorder="little")
    s = argmin(m)[:, None]
    path = np.zeros((B, T), np.float32)
    for t in range(T - 1, -1, -1):
        s = (2 * s + take1[rows, t, s]) % S
        path[:, t] = (s & 1)[:, 0]
    return dec, m, surv, path


# Seeds found by a CPU search (the first that pass; with the densities above some seeds give too few ties at some shape): for
# every (B, T) of TIE_SHAPES[S] and both `strict` values they meet the preconditions that test_exact_nets_host.py asserts.
TIE_SEEDS = {(2, True): 2, (2, False): 1, (4, True): 19, (4, False): 4, (8, True): 2, (8, False): 1, (16, True): 4, (16, False): 1,
             (32, True): 2, (32, False): 1, (64, True): 3, (64, False): 5, (128, True): 2, (128, False): 1, (256, True): 1,
             (256, False): 1}
TIE_SHAPES = {S: [(9, 75), (5, 33)] for S in (2, 4, 8, 16, 32, 64, 128, 256)}
TIE_SHAPES[4] += [(70, 72)]
TIE_SHAPES[64] += [(70, 72)]
TIE_SHAPES[16] += [(70, 72), (5, 136), (3, 200), (801, 31), (1100, 72), (7000, 40)]


def _tie_inputs(S, fast, strict, B, T):
    rng = np.random.RandomState(TIE_SEEDS[S, fast])
    w = staircase_weights(S, rng, fast, strict)
    y = np.random.RandomState(TIE_SEEDS[S, fast] + 1000 * B + T).choice(GRID_FAST if fast else GRID_SLOW, (B, T))
    return w, np.ascontiguousarray(y, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def tie_case(S, fast, strict, B, T):
    """One tie-heavy input and its NumPy reference, computed once and shared (treat the arrays as read-only):
    dict(w, y, logits f32 [B, T, S], dec, fm, surv, path)."""
    w, y = _tie_inputs(S, fast, strict, B, T)
    lg64 = ideal_logits(y, w)
    logits = lg64.astype(np.float32)
    assert np.array_equal(logits, lg64) and np.array_equal(lg64 * 4, np.round(lg64 * 4))  # multiples of 1/4, exact in f32
    dec, fm, surv, path = textbook_acs(-logits)
    return dict(w=w, y=y, logits=logits, dec=dec, fm=fm, surv=surv, path=path)


def tie_preconditions(S, fast, strict, B, T):
    """What makes tie_case able to catch a wrong tie rule, from the NumPy reference alone: the shares of decisions after symbol 0
    and of survivor bits that differ between first-index and last-index tie breaking, the share of decisions that are 1, and
    4 T max|logit| (below 2^24: every path metric is exact in f32)."""
    c = tie_case(S, fast, strict, B, T)
    dec_l, fm_l, surv_l, _ = textbook_acs(-c["logits"], last=True)
    assert np.array_equal(fm_l, c["fm"])  # the tie rule picks an index, never a value
    sb = np.unpackbits(c["surv"], axis=2, bitorder="little")[:, :, :S]
    sb_l = np.unpackbits(surv_l, axis=2, bitorder="little")[:, :, :S]
    return dict(dec_ties=float(np.mean(c["dec"][:, 1:] != dec_l[:, 1:])), surv_ties=float(np.mean(sb != sb_l)),
                ones=float(np.mean(c["dec"][:, 1:])), exact=4.0 * T * float(np.abs(c["logits"]).max()))


# ---- sigmoid range ---------------------------------------------------------------------------------------------------------
LADDER_WMAX, LADDER_BMAX = 8.0, 6.0
LADDER_RUNGS = [85.9, 86.0, 86.1, 87.5, 88.5, 95.0, 104.5, 130.0, 1e6, 3e38]  # values of max|y| max|W1| + max|b1| of a tile
_RUNG_TILES = [(0, 2), (1, 1), (2, 3), (3, 0), (4, 4), (6, 5), (8, 6), (10, 7), (12, 8), (14, 9)]  # row 0: (16-symbol tile, rung)


def ladder_weights(S, rng):
    """Random-uniform weights like the suite's other ViterbiNet tests, W1 and b1 rescaled to max|W1| = 8 and max|b1| = 6, both
    maxima on ONE hidden-1 unit, its bias negative: a rung sample of the right sign puts that unit's sigmoid argument on -rung."""
    w = [rng.uniform(-1, 1, (H1, 1)), rng.uniform(-1, 1, H1), rng.uniform(-0.1, 0.1, (H2, H1)), rng.uniform(-0.1, 0.1, H2),
         rng.uniform(-0.14, 0.14, (S, H2)), rng.uniform(-0.14, 0.14, S)]
    w[0] *= LADDER_WMAX / np.abs(w[0]).max()
    w[1] *= 0.9 * LADDER_BMAX / np.abs(w[1]).max()
    k = int(np.argmax(np.abs(w[0])))
    w[1][k] = -LADDER_BMAX
    w = [np.ascontiguousarray(x, dtype=np.float32) for x in w]
    assert np.abs(w[0]).max() == LADDER_WMAX and np.abs(w[1]).max() == LADDER_BMAX
    return w


def ladder_samples(B, T, rng):
    """y ~ N(0, 1.3) with 3 % of the samples of rows >= 1 (at least one per value) replaced by +-(rung - 6) / 8, by -0.0 or by 1e-40.  Row 0 is laid out by
    hand (_RUNG_TILES, as far as T reaches): a tile holds its rung with either sign among ordinary samples; the slow rungs (86.1,
    87.5, 88.5 ...) sit in even tiles, 86.0 and 85.9 -- still the fast form -- and ordinary tiles in between."""
    y = rng.normal(0, 1.3, (B, T))
    special = [(r - LADDER_BMAX) / LADDER_WMAX for r in LADDER_RUNGS]
    pool = np.array(special + [-s for s in special] + [-0.0, 1e-40])
    if B > 1:  # (the pool is dealt out in turn, so every value occurs once there are len(pool) replacements)
        n = min((B - 1) * T, max(int(np.ceil(0.03 * (B - 1) * T)), len(pool)))
        hit = rng.choice((B - 1) * T, n, replace=False)
        y[1:].reshape(-1)[hit] = pool[np.arange(n) % len(pool)]
    y[0] = np.clip(y[0], -5.0, 5.0)
    for tile, r in _RUNG_TILES:
        if 16 * tile + 9 < T:
            y[0, 16 * tile + 5], y[0, 16 * tile + 9] = special[r], -special[r]
    return np.ascontiguousarray(y, dtype=np.float32)


# ---- the subnormal pin -----------------------------------------------------------------------------------------------------
SUBNORMAL_KJ = [(k, j) for k in (0, 3, 99) for j in (5, 47, 48, 49)]
TWO40 = np.float32(2.0 ** 40)  # < kStrictMinBound


def subnormal_net(S, k, j, rng):
    """Hidden-1 unit k: W1 = -88, b1 = 0, so y = 1.0 gives sigmoid(-88) = 6.05e-39, a subnormal float (y = 0.5: 7.8e-20).  Hidden-2
    unit j sees unit k alone (W2[j, k] = 2^40, b2[j] = 0) and the states with bit 1 set (half of them) see unit j alone (W3[s, j] =
    2^40, b3[s] = 0): their logit is 2^80 sigmoid(-88 y), 7.3e-15 where a flushed activation would give 0.  State 0's logit is
    exactly 0 and the remaining states' logits are about -8, so in a block of y = 1.0 alone the odd states -- whose predecessors
    have bit 1 set -- lead by 7.3e-15 per symbol and every decision after symbol 0 is 1; with a flushed activation state 0 ties
    them and the decisions are 0.  S >= 4."""
    w = [rng.uniform(-0.5, 0.5, (H1, 1)), rng.uniform(-0.5, 0.5, H1), rng.uniform(-0.1, 0.1, (H2, H1)), rng.uniform(-0.1, 0.1, H2),
         rng.uniform(-0.14, 0.14, (S, H2)), np.full(S, -8.0)]
    w[0][k, 0], w[1][k] = -88.0, 0.0
    w[2][j, :], w[3][j] = 0.0, 0.0
    w[2][j, k] = TWO40
    w[4][:, j] = 0.0
    half = (np.arange(S) & 2) != 0
    w[4][half, :], w[5][half] = 0.0, 0.0
    w[4][half, j] = TWO40
    w[4][0, :], w[5][0] = 0.0, 0.0
    return [np.ascontiguousarray(x, dtype=np.float32) for x in w]


def flushed(w, k, j):
    """The same network with the path from hidden-1 unit k to hidden-2 unit j cut: what flushing h1[k] to 0 would compute."""
    w = [x.copy() for x in w]
    w[2][j, k] = 0.0
    return w


def subnormal_samples(B, T, rng):
    """y = 1.0 and 0.5 mixed; row 0 is 1.0 throughout and the last row holds whole 32-symbol stretches of 0.5 (fast-form tiles)."""
    y = rng.choice([1.0, 0.5], (B, T))
    y[0] = 1.0
    if B > 1:
        y[B - 1] = np.where((np.arange(T) // 32) % 2 == 0, 0.5, y[B - 1])
    return np.ascontiguousarray(y, dtype=np.float32)
