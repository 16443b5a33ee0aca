"""CPU checks of tests/sigmoid_sweep.py, which test_gpu_sigmoid_sweep.py relies on: the probe networks are transparent (the
oracle's logits and final metrics of them ARE 2^40 oracle.sigmoid(c y), bit for bit); the sets cover what they claim, from the
arrays alone; the fast / slow form of each network follows from the kernels' rule; and the referee itself -- oracle.sigmoid, the
C restatement that every ViterbiNet kernel is held to -- equals torch.sigmoid bit for bit over the same sweep and stays within
its derived bound of the float64 sigmoid.  No GPU."""
import numpy as np
import pytest
import torch

import sigmoid_sweep as W

FORMS = pytest.mark.parametrize("slow", [False, True], ids=["fast", "slow"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sample(y, n=100000):
    """n samples of a set, its two ends among them, and every special value."""
    return np.concatenate([y[np.unique(np.linspace(0, y.size - 1, n).astype(np.int64))], W.SPECIALS])


# ---------------------------------------------------------------- 1. transparency
@pytest.mark.parametrize("name", list(W.SETS))
@FORMS
@pytest.mark.parametrize("S", [4, 16, 32])
def test_probe_net_logits_are_the_sigmoids_bits(oracle, S, slow, name):
    """oracle.vnet_logits(probe_net) == float32(2^40 oracle.sigmoid(float32(c) float32(y))) on 1e5 samples of each set and all
    specials, for the plain network and the slow twin; states past the 16 probes hold +0."""
    y = _sample(W.SETS[name])
    want = W.expected_logits(W.expected(oracle, y), S)
    got = oracle.vnet_logits(y, W.probe_net(S, slow))
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(want).all() and want.max() <= W.TWO40 and not np.signbit(want).any()


@pytest.mark.parametrize("name", list(W.SETS))
@FORMS
@pytest.mark.parametrize("S", [4, 16, 128])
def test_final_metric_net_returns_the_sigmoids_bits(oracle, S, slow, name):
    """Blocks of one symbol through oracle.vnet_decode: final_metric[s] = 0 - 2^40 sigmoid(c y) of probe s mod S/2 (+0 where the
    sigmoid is 0, and for the states past the probes), every decision 0."""
    y = _sample(W.SETS[name], 20000)
    dec, fm = oracle.vnet_decode(y.reshape(-1, 1), W.final_metric_net(S, slow), want_final=True)
    want = W.expected_final(W.expected(oracle, y), S)
    assert np.array_equal(_bits(fm), _bits(want)) and not dec.any()
    assert not np.signbit(want[want == 0]).any() and (want <= 0).all()


# ---------------------------------------------------------------- 2. coverage
def test_fast_exhaustive_holds_every_float_and_every_q():
    """Every float of [43, 86] (by size and by consecutive bit patterns), and over the 16 probes all 249 values -124 ... 124 of the
    range-reduction integer q (z = c y is monotonic in y, and so is q: its distinct values are where it steps)."""
    y = W.FAST_EXHAUSTIVE
    assert y.size == 8388609 and y[0] == 43.0 and y[-1] == 86.0
    assert np.all(np.diff(_bits(y).astype(np.int64)) == 1)
    seen = set()
    zmin = np.inf
    for c in W.PROBE_C:
        q = W.range_reduction_q(c * y)
        assert np.all(np.abs(np.diff(q)) <= 1)
        seen.update(q[np.flatnonzero(np.diff(q)) + 1].tolist() + [int(q[0])])
        zmin = min(zmin, float(np.abs(c * y).min()))
    assert seen == set(range(-124, 125)) and zmin == 0.3359375
    # the probes' ranges of |z| join up (43 * 2^-i <= 86 * 2^-(i+1)): every float with 0.3359375 <= |z| <= 86 is an argument
    assert np.array_equal(np.abs(W.PROBE_C[::2]), 2.0 ** -np.arange(8.0)) and np.array_equal(W.PROBE_C[1::2], -W.PROBE_C[::2])


def test_sets_have_the_sizes_and_ends_they_claim():
    assert W.WINDOW.size == 393217 and W.WINDOW[0] == 86.0 and W.WINDOW[-1] == 89.0
    assert np.all(np.diff(_bits(W.WINDOW).astype(np.int64)) == 1)
    wide = W.WIDE_STRIDED[:-W.SPECIALS.size]
    assert wide.size == 16 * (1 << 23) // 64 + 1 and wide[0] == np.float32(86.0 * 2.0 ** -16) and wide[-1] == 86.0
    assert np.all(np.diff(_bits(wide).astype(np.int64)) == 64)
    assert set(np.frexp(wide[:-1])[1].tolist()) == set(range(-9, 7 + 1))  # 86 * 2^-16 ... 86: 15 whole binades and a part of one at each end
    far = W.FAR[:-1]
    assert far[0] == 89.0 and np.all(np.diff(_bits(far).astype(np.int64)) == 4096) and W.FAR[-1] == W.FLT_MAX
    assert 2.4e5 < W.FAR.size < 2.6e5 and np.isfinite(W.FAR).all()
    assert _bits(W.SPECIALS).size == len(set(_bits(W.SPECIALS).tolist())) == 8


def test_window_holds_the_subnormal_sigmoids(oracle):
    """sigmoid(-y) over WINDOW: normal values, at least 181 704 subnormal ones (all there are: every float of the window is in the
    set) and exact zeros; and over FAST_EXHAUSTIVE's probe of c = 1/4 the step to exactly 1.0 (from z = 16.635532 on)."""
    s = oracle.sigmoid(-W.WINDOW)
    tiny = np.float32(2.0 ** -126)
    sub = (s > 0) & (s < tiny)
    assert int(sub.sum()) >= 181704 and (s == 0).any() and (s >= tiny).any()
    assert np.all(np.diff(s) <= 0) and s[-1] == 0 and not np.signbit(s).any()
    first0 = W.WINDOW[np.argmax(s == 0)]
    assert abs(float(first0) - 88.72284) < 1e-4
    z = np.float32(0.25) * W.FAST_EXHAUSTIVE
    s = oracle.sigmoid(z)
    assert (s == 1.0).any() and (s < 1.0).any() and s.max() == 1.0
    assert z[np.argmax(s == 1.0)] == np.float32(16.635532)


# ---------------------------------------------------------------- 3. the form rule
@pytest.mark.parametrize("S", [4, 16, 256])
def test_form_rule(S):
    """max|y| max|W1| + max|b1| in float32 (the kernels' test, per tile or unit): <= 86 on every fast set with the plain networks,
    > 86 on every set with the slow twins, > 86 for all of WINDOW and FAR but WINDOW's first sample either way."""
    for net in (W.probe_net, W.final_metric_net):
        plain, twin = net(S), net(S, True)
        assert np.abs(plain[0]).max() == 1.0 and np.abs(plain[1]).max() == 0.0 and np.abs(twin[1]).max() == 100.0
        assert not twin[2][:, W.TWIN_K].any() and twin[0][W.TWIN_K, 0] == 0
        for y in W.FAST_SETS.values():
            assert W.form_bound(y, plain) <= W.FAST_BOUND
            assert W.form_bound(y[:1], twin) > W.FAST_BOUND  # (already for the smallest sample)
        for y in (W.WINDOW[1:2], W.FAR[:1]):
            assert W.form_bound(y, plain) > W.FAST_BOUND


# ---------------------------------------------------------------- 4. the referee against torch
def _whole_range():
    pos = np.arange(0, W._bits(W.FLT_MAX) + 1, 61, dtype=np.uint32).view(np.float32)
    return np.concatenate([pos, -pos])


def _referee_arguments():
    both = lambda a: np.concatenate([a, -a])
    return {"fast_exhaustive": both(W.FAST_EXHAUSTIVE), "window": both(W.WINDOW), "far": both(W.FAR), "every_61st": _whole_range()}


# ATen's vectorised sigmoid is one source compiled per capability.  AVX512 is what the goldens' torch build runs on; AVX2 was
# run over the same four sets (ATEN_CPU_CAPABILITY=avx2) and agrees in every value, so it is admitted.
ADMITTED = ("AVX512", "AVX2")


@pytest.mark.parametrize("name", ["fast_exhaustive", "window", "far", "every_61st"])
def test_oracle_sigmoid_equals_torch_sigmoid(oracle, name):
    """oracle.sigmoid == torch.sigmoid bit for bit (CPU, one thread, a multiple of 64 values so that ATen's vectorised loop covers
    all of them): the +-1 arguments of FAST_EXHAUSTIVE, WINDOW and FAR in both signs, every 61st float of the finite range in both
    signs.  The golden logits tie the two together over |z| < 10 only.  A difference here is a finding about the oracle."""
    cap = torch.backends.cpu.get_cpu_capability()
    if cap not in ADMITTED:
        pytest.skip(f"torch CPU capability {cap}: the comparison is established for {' and '.join(ADMITTED)}")
    z = _referee_arguments()[name]
    z = np.ascontiguousarray(z[:z.size - z.size % 64])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = torch.sigmoid(torch.from_numpy(z)).numpy()
    finally:
        torch.set_num_threads(threads)
    o = oracle.sigmoid(z)
    bad = np.flatnonzero(_bits(t) != _bits(o))
    assert bad.size == 0, (cap, bad.size, z[bad[:4]].tolist(), t[bad[:4]].tolist(), o[bad[:4]].tolist())


# ---------------------------------------------------------------- 5. the referee against float64
@pytest.mark.parametrize("name", ["fast_exhaustive", "window", "far", "every_61st"])
def test_oracle_sigmoid_within_its_bound_of_float64(oracle, name):
    """Where the result is a normal float: |oracle.sigmoid(z) - 1 / (1 + exp(-z))| <= 2^-22 of the float64 value.  Derived, not
    tuned: expf_u10 is within 1 ulp (2^-23 relative) of e = exp(-z), which moves 1 / (1 + e) by at most 2^-23 e / (1 + e) < 2^-23
    relative; the sum 1 + e and the quotient round once each, 2^-24 relative apiece: 2^-22 in all.  (Measured: at most 2.40 2^-24.)"""
    z = _referee_arguments()[name]
    o = oracle.sigmoid(z)
    with np.errstate(over="ignore"):
        ref = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    normal = np.abs(o) >= np.float32(2.0 ** -126)
    assert normal.any()
    err = np.abs(o[normal].astype(np.float64) - ref[normal]) / ref[normal]
    worst = float(err.max())
    print(f"{name}: {int(normal.sum())} normal results, largest relative error {worst * 2.0 ** 24:.3f} * 2^-24")
    assert worst <= 2.0 ** -22
