"""Networks whose logits ARE the bits of the ViterbiNet sigmoid, the sets of samples that sweep its whole argument range, and
the expectation they are compared with.  CPU only; imported by test_sigmoid_sweep_host.py and test_gpu_sigmoid_sweep.py.

  probe_net / final_metric_net
      Probe i sits on hidden-1 unit PROBE_K[i] (W1 = PROBE_C[i], b1 = 0), hidden-2 unit PROBE_J[i] (W2 = 2^40) and one state
      (W3 = 1); everything else is zero, so every other product of the k-ordered chains is an exact zero and
      logit[state] = 2^40 sigmoid(fl(c y)) bit for bit.  2^40 (exact_nets.subnormal_net's factor) keeps a subnormal activation's
      product normal and stays below kStrictMinBound and below the cost sweeps' 1e18.  slow = True adds b1 = -100 on one
      unit nothing reads: the bound max|y| max|W1| + max|b1| is past 86 and every tile takes the IEEE-division form.
  FAST_EXHAUSTIVE / WIDE_STRIDED / WINDOW / FAR
      Samples y > 0 (the probes carry both signs); with max|W1| = 1 and max|b1| = 0 a tile is fast exactly when max|y| <= 86.
  expected / expected_final
      float32(2^40 oracle.sigmoid(float32(c) float32(y))): one table per chunk of samples, for every route and both forms.
"""
import numpy as np

H1, H2 = 100, 50
TWO40 = np.float32(2.0 ** 40)
FAST_BOUND = np.float32(86.0)  # kFastSigmoidBound
# probe 2i: +2^-i, probe 2i+1: -2^-i: the first S probes of a network with fewer states still hold both signs
PROBE_C = np.array([s * 2.0 ** -i for i in range(8) for s in (1.0, -1.0)], np.float32)
PROBE_K = (0, 99, 3, 50, 7, 96, 13, 22, 31, 37, 44, 58, 63, 71, 85, 92)  # hidden-1 units, all over 0 ... 99
# hidden-2 units: the MFMA row tiles' ends and middles and the two fmaf-chain units 48 and 49 (within the first four probes, which
# is all that a 4-state network has)
PROBE_J = (5, 47, 48, 49, 0, 15, 16, 31, 32, 20, 27, 36, 41, 10, 45, 2)
TWIN_K, TWIN_B1 = 1, np.float32(-100.0)  # the slow twin's unit (no probe, its W2 column zero)
BLOCK_T = 1024
MAX_LOGIT_FLOATS = 1 << 25  # per launch: 2^21 symbols at 16 states, 134 MB


def _empty(S):
    return [np.zeros((H1, 1), np.float32), np.zeros(H1, np.float32), np.zeros((H2, H1), np.float32), np.zeros(H2, np.float32),
            np.zeros((S, H2), np.float32), np.zeros(S, np.float32)]


def _probes(w, n, slow):
    for i in range(n):
        w[0][PROBE_K[i], 0] = PROBE_C[i]
        w[2][PROBE_J[i], PROBE_K[i]] = TWO40
    if slow:
        assert TWIN_K not in PROBE_K
        w[1][TWIN_K] = TWIN_B1
    return w


def n_probes(S):
    return min(S, 16)


def probe_net(S, slow=False):
    """[W1, b1, W2, b2, W3, b3] with logit[i] = 2^40 sigmoid(fl(PROBE_C[i] y)) for i < min(S, 16); the other states' logits are +0."""
    w = _probes(_empty(S), n_probes(S), slow)
    for i in range(n_probes(S)):
        w[4][i, PROBE_J[i]] = 1.0
    return w


def n_final_probes(S):
    return min(S // 2, 8)


def final_metric_net(S, slow=False):
    """For kernels that write no logits, run on blocks of T = 1: states 2i and 2i+1 both carry probe i (i < min(S/2, 8)), so both
    candidates of every state are equal and final_metric[s] = 0 - logit[2s mod S] whatever the minimum's tie rule."""
    w = _probes(_empty(S), n_final_probes(S), slow)
    for i in range(n_final_probes(S)):
        w[4][2 * i, PROBE_J[i]] = w[4][2 * i + 1, PROBE_J[i]] = 1.0
    return w


def form_bound(y, w):
    """max|y| max|W1| + max|b1| as the kernels evaluate it (float32, two roundings)."""
    return np.float32(np.float32(np.abs(y).max() * np.abs(w[0]).max()) + np.abs(w[1]).max())


# ---- the sets ----------------------------------------------------------------------------------------------------------------
def _bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def floats(lo, hi, stride=1):
    """Every stride-th float32 of [lo, hi] (0 < lo <= hi), from lo on."""
    return np.arange(_bits(lo), _bits(hi) + 1, stride, dtype=np.uint32).view(np.float32)


FLT_MAX = np.finfo(np.float32).max
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -126, -2.0 ** -126, 1e-30, -1e-30], np.float32)
FAST_EXHAUSTIVE = floats(43.0, 86.0)  # with the 16 probes: every float z with 0.3359375 <= |z| <= 86
WIDE_STRIDED = np.concatenate([floats(86.0 * 2.0 ** -16, 86.0, 64), SPECIALS])  # +-1 probes alone: all 16 binades
WINDOW = floats(86.0, 89.0)  # sigmoid(-y) a subnormal float in (87.33655, 88.72284), 0 from there on
FAR = np.concatenate([floats(89.0, FLT_MAX, 4096), np.array([FLT_MAX], np.float32)])  # exp's clamps and beyond
STRIDED = np.concatenate([WIDE_STRIDED, WINDOW[::8], FAR])  # what every route gets: fast units, then slow ones
FINAL_STRIDED = np.concatenate([WIDE_STRIDED, WINDOW[::8]])
FAST_SETS = {"FAST_EXHAUSTIVE": FAST_EXHAUSTIVE, "WIDE_STRIDED": WIDE_STRIDED}
SETS = dict(FAST_SETS, WINDOW=WINDOW, FAR=FAR)


def blocks(y, T=BLOCK_T):
    """[B, T], the last block padded with the last sample."""
    B = -(-y.size // T)
    return np.ascontiguousarray(np.concatenate([y, np.full(B * T - y.size, y[-1], np.float32)]).reshape(B, T))


def chunks(n, most):
    """[(start, stop)]: 0 ... n in the fewest pieces of at most `most`, of even size."""
    k = -(-n // most)
    edges = [n * i // k for i in range(k + 1)]
    return list(zip(edges[:-1], edges[1:]))


def range_reduction_q(z):
    """q = rint(-z log2 e) as both forms of the sigmoid compute it (float32 product, ties to even)."""
    return np.rint(-np.asarray(z, np.float32) * np.float32(1.4426950408889634)).astype(np.int64)


# ---- the expectation ---------------------------------------------------------------------------------------------------------
def expected(oracle, y, P=16):
    """[y.size, P] float32: 2^40 oracle.sigmoid(fl(PROBE_C[p] y)), the logits of probe_net's first P states."""
    z = np.asarray(y, np.float32).reshape(-1, 1) * PROBE_C[:P]
    assert z.dtype == np.float32
    return TWO40 * oracle.sigmoid(z)


def expected_logits(table, S):
    """probe_net(S)'s logits [N, S] from expected(...)'s table [N, >= min(S, 16)]."""
    out = np.zeros((table.shape[0], S), np.float32)
    out[:, :n_probes(S)] = table[:, :n_probes(S)]
    return out


def expected_final(table, S):
    """final_metric_net(S)'s final metrics [N, S] on blocks of one symbol: 0 - logit[2s mod S] (+0 where the sigmoid is 0)."""
    P = n_final_probes(S)
    logit = np.zeros((table.shape[0], S), np.float32)
    logit[:, :2 * P] = np.repeat(table[:, :P], 2, axis=1)
    return np.float32(0.0) - logit[:, (2 * np.arange(S)) % S]
