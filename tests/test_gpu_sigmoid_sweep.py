"""GPU tests (pytest -m gpu): the ViterbiNet sigmoid over its whole argument range, bit for bit, in both of its forms
(sigmoid_from_neg: expf_u10, ldexpf, IEEE division; sigmoid_from_neg_fast: magic-number exponent, v_rcp_f32 + one Newton step).
The networks of tests/sigmoid_sweep.py turn a kernel's logits (or, for a kernel that writes none, its final metrics) into
2^40 sigmoid(c y); the expectation is float32(2^40 oracle.sigmoid(float32(c) float32(y))), computed once per chunk of samples and
compared on the device for every route and both forms.  test_sigmoid_sweep_host.py shows on the CPU that the networks are
transparent, that the sets cover what they claim and that oracle.sigmoid is torch.sigmoid.  No tolerance anywhere.

  test_sigmoid_exhaustive        every float z with 0.3359375 <= |z| <= 86 (all 249 values of the range-reduction integer q, both
                                 neighbours of each of its switch points) and every float of [86, 89] (the subnormal results and
                                 the step to 0), through vnet16_dealt_kernel<true> and vnet16_fusedn_kernel<true, 2>
  test_sigmoid_every_route       16 binades below 86, every 8th float of [86, 89] and the range up to the largest float through
                                 every route of SIGMOID_ROUTES; test_sigmoid_logits_entry: mvn_vnet_logits_f32 itself
  test_sigmoid_final_metrics     the 16-state kernels that write no logits, on blocks of one symbol

What blocks of one symbol cannot reach: a final metric is the sigmoid's bits only after ONE stage, so the decision-only kernels
(vnet16_dealt_ring1_kernel, vnet16_dealt_kernel<false>, vnet16_fusedn_kernel<false, NT>, vnet_fused_ip_kernel<LB>) are observed
in the one-tile k-loop of a block's last unit alone.  Their two-tile instantiation (and vnet_fused_ip_kernel's whole chunks) call
the same two functions and stay pinned through the existing tests that hold their decisions equal to the logits routes'.

What these tests were seen to catch (edits tried on a scratch build, never committed, like those at the top of
test_gpu_exact_nets.py; the whole GPU suite but its long replay, multi-process and full-configuration tests was run on each build).
(1) sigmoid_from_neg_fast returning v_rcp_f32's value without the Newton step: 9 % of the logits differ (2 402 422 of the
26 836 992 of FAST_EXHAUSTIVE's first chunk).  test_sigmoid_exhaustive[FAST_EXHAUSTIVE], the nine routes of
test_sigmoid_every_route that have a fast form and all of test_sigmoid_final_metrics fail; the six mlp_kernel routes and
test_sigmoid_logits_entry (the slow form only) pass, as they must.  Random weights notice this edit too: 176 existing cases fail
(test_vnet_golden_bit_exact, test_vnet_vs_oracle, test_vnet16_dealt_kernel_vs_oracle, test_vnet16_fused_and_unfused_paths,
test_vnet_fused_ip_and_two_kernel_routes, test_vnet_partial_nan_follows_torch_min, test_ring1_decisions_and_final_metrics, both
sigmoid tests of test_gpu_exact_nets.py, test_gpu_list_step.py, test_gpu_graph_replay.py, ...).
(2) The low word of ln 2 in sigmoid_from_neg_fast's range reduction one ulp off (-1.4286068790170248e-06f), an error that grows
with |q|: 13 of the 26 853 376 logits of FAST_EXHAUSTIVE's second chunk differ (first at y = 49.899109, c = 1) and 3 of STRIDED's
(y = 49.9140625, 76.96044921875, 76.96923828125).  The same 13 cases fail as in (1) -- and NOTHING else in the suite.
(3) sigmoid_from_neg flushing a subnormal quotient to 0: exactly WINDOW's 181 704 subnormal results differ (first at
y = 87.336548) and 23 028 of STRIDED's.  test_sigmoid_exhaustive[WINDOW], all 15 routes, test_sigmoid_logits_entry and
test_sigmoid_final_metrics fail; of the existing tests test_vnet_subnormal_activation_is_kept (its one argument, -88) fails in all
180 cases and test_vnet_sigmoid_range_ladder, whose subnormal activations meet weights of 0.1, does not notice.
"""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import sigmoid_sweep as W
from test_gpu_exact_nets import SIGMOID_IDS, SIGMOID_ROUTES, _kernel_name
from test_gpu_parity import _weights_t

pytestmark = pytest.mark.gpu

FORMS = [(False, "fast"), (True, "slow")]  # (the slow twin?, what the plain network's form is called on a fast set)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


_tables = {}


def _strided_table(oracle):
    """expected(STRIDED) for all 16 probes, computed once for the module (read-only): [2.4e6, 16]."""
    if "strided" not in _tables:
        _tables["strided"] = W.expected(oracle, W.STRIDED)
    return _tables["strided"]


def _rows(a, r0, r1):
    """Rows r0 ... r1 - 1 of a [N, ...] (or [N]) array, its last row repeated past its end: the padding of the last block."""
    n = a.shape[0]
    assert r0 < n
    return a[r0:r1] if r1 <= n else np.concatenate([a[r0:n], np.repeat(a[n - 1:n], r1 - n, axis=0)])


def _launch(lib, dev, yt, wt, S, want_logits):
    """mvn_vnet_decode_f32 with the workspace the library asks for (the two-kernel route puts its logits into logits_out)."""
    B, T = yt.shape
    dec, fm = torch.full((B, T), 7.0, device=dev), torch.empty(B, S, device=dev)
    lg = torch.empty(B, T, S, device=dev) if want_logits else None
    nb = int(lib.mvn_vnet_workspace_bytes(B, T, S))
    if nb == B * T * S * 4:
        assert want_logits
        nb = 0
    ws = torch.full((max(nb, 4),), 0x5A, dtype=torch.uint8, device=dev)  # (stale contents: the launch clears what it uses)
    rc = lib.mvn_vnet_decode_f32(mvn._lib.ptr(yt), T, *[mvn._lib.ptr(t) for t in wt], mvn._lib.ptr(dec), T, mvn._lib.ptr(lg),
                                 mvn._lib.ptr(fm), mvn._lib.ptr(ws), nb, B, T, S, mvn._lib.current_stream(dev))
    assert rc == 0
    status = int(ws[:4].view(torch.int32).item()) if nb else 0  # the dealt kernel's status word: a hand-off abandoned
    return dec, lg, fm, nb, status


def _assert_same_bits(got, want, y, what):
    """got == want as bit patterns, compared on the device; got / want [N, P], y [N] the samples (for the message)."""
    g, w = got.view(torch.int32), want.view(torch.int32)
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero()
    r, c = bad[:4, 0], bad[:4, 1]
    pytest.fail(f"{what}: {bad.shape[0]} of {g.numel()} values differ; first at y = {y.reshape(-1)[r].tolist()}, columns {c.tolist()}: "
                f"got {got[r, c].tolist()}, expected {want[r, c].tolist()}")


def _check_logits(lg, want, yt, S, what):
    P = W.n_probes(S)
    lg = lg.view(-1, S)
    _assert_same_bits(lg[:, :P], want[:, :P], yt, what)
    if S > P:
        assert not bool(lg[:, P:].view(torch.int32).any()), (what, "a state past the probes is not +0")


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _delenv(monkeypatch, env):
    for k in env:
        monkeypatch.delenv(k)


# ---------------------------------------------------------------- exhaustive
EXHAUSTIVE_ROUTES = [({}, "vnet16_dealt_kernel<true> rings of "), ({"MVN_DEALT": "0", "MVN_COOP": "0"}, "vnet16_fusedn_kernel<true, 2>")]


@pytest.mark.parametrize("name", ["FAST_EXHAUSTIVE", "WINDOW"])
def test_sigmoid_exhaustive(oracle, dev, monkeypatch, name):
    """Every sample of the set in [B, 1024] blocks, at most 2^21 symbols per launch, through the default 16-state call and the
    one-wave-per-block kernel, on the probe network (FAST_EXHAUSTIVE: the fast form; WINDOW: the kernel leaves it by itself) and
    on the slow twin: all 16 logits of every symbol are the expectation's bits."""
    lib, S = mvn._lib.load(), 16
    yb = W.blocks(W.SETS[name])
    nets = [_weights_t(W.probe_net(S, slow), dev) for slow, _ in FORMS]
    for b0, b1 in W.chunks(yb.shape[0], W.MAX_LOGIT_FLOATS // (W.BLOCK_T * S)):
        want = torch.from_numpy(W.expected(oracle, yb[b0:b1])).to(dev)
        yt = torch.from_numpy(yb[b0:b1]).to(dev)
        for env, kernel in EXHAUSTIVE_ROUTES:
            _setenv(monkeypatch, env)
            what = (name, _kernel_name(lib, b1 - b0, W.BLOCK_T, S, True), b0, b1)
            assert what[1].startswith(kernel), what
            for wt, (slow, form) in zip(nets, FORMS):
                _, lg, _, nb, status = _launch(lib, dev, yt, wt, S, True)
                assert (nb > 0) == ("dealt" in kernel) and status == 0, what
                _check_logits(lg, want, yt, S, what + ("slow twin" if slow else "probe network",))
                del lg
            _delenv(monkeypatch, env)


# ---------------------------------------------------------------- every route, strided
def _plan(S, env, dealt):
    """(block length, logits written?, what the kernel-name query must answer) for an entry of SIGMOID_ROUTES.  The three entries
    that run the dealt kernel get blocks of three lengths, so that the launch plans differ (rings of 8, of fewer, of 1)."""
    if env.get("MVN_FUSED_IP") == "1":
        return 1, False, f"vnet_fused_ip_kernel<{S.bit_length() - 3}>"
    if env.get("MVN_UNFUSED") == "1":
        return W.BLOCK_T, True, f"mlp_kernel<{(S + 15) // 16}> + "
    if env.get("MVN_COOP") == "1":
        return W.BLOCK_T, True, "vnet16_coop_kernel<true>"
    if "MVN_FUSEDN" in env or env.get("MVN_DEALT") == "0":
        return W.BLOCK_T, True, f"vnet16_fusedn_kernel<true, {env.get('MVN_FUSEDN', '2')}>"
    return (W.BLOCK_T if not dealt else 352 if env else 128), True, "vnet16_dealt_kernel<true> rings of "


@pytest.mark.parametrize("S,env,shapes,dealt", SIGMOID_ROUTES, ids=SIGMOID_IDS)
def test_sigmoid_every_route(oracle, dev, monkeypatch, S, env, shapes, dealt):
    """STRIDED (every 64th float of the 16 binades below 86 and the special samples, every 8th float of [86, 89], every 4096th up
    to the largest float) through every route of SIGMOID_ROUTES, on the plain network and the slow twin.  Routes that write
    logits: all min(S, 16) probes' logits, +0 in the other states.  vnet_fused_ip_kernel<LB> writes none: blocks of one symbol on
    final_metric_net, min(S / 2, 8) probes through the final metrics, every decision 0."""
    _setenv(monkeypatch, env)
    lib = mvn._lib.load()
    T, logits, kernel = _plan(S, env, dealt)
    table = _strided_table(oracle)
    yb = W.blocks(W.STRIDED, T)
    nets = [_weights_t((W.probe_net if logits else W.final_metric_net)(S, slow), dev) for slow, _ in FORMS]
    for b0, b1 in W.chunks(yb.shape[0], max(1, W.MAX_LOGIT_FLOATS // (T * S))):
        rows = _rows(table, b0 * T, b1 * T)
        want = torch.from_numpy(np.ascontiguousarray(rows[:, :W.n_probes(S)]) if logits else W.expected_final(rows, S)).to(dev)
        yt = torch.from_numpy(yb[b0:b1]).to(dev)
        what = (_kernel_name(lib, b1 - b0, T, S, logits), b0, b1)
        assert what[0].startswith(kernel), what
        for wt, (slow, _) in zip(nets, FORMS):
            dec, lg, fm, nb, status = _launch(lib, dev, yt, wt, S, logits)
            assert (nb > 0) == ("dealt" in kernel) and status == 0, what
            if logits:
                _check_logits(lg, want, yt, S, what + (slow,))
            else:
                _assert_same_bits(fm, want, yt, what + (slow,))
                assert not bool(dec.any()), what
            del lg, fm


@pytest.mark.parametrize("S", [2, 16, 64])
def test_sigmoid_logits_entry(oracle, dev, S):
    """mvn_vnet_logits_f32 (mlp_kernel: the slow form throughout) on STRIDED, both networks."""
    lib = mvn._lib.load()
    table = _strided_table(oracle)
    n = W.MAX_LOGIT_FLOATS // S
    for slow, _ in FORMS:
        wt = _weights_t(W.probe_net(S, slow), dev)
        for r0, r1 in W.chunks(W.STRIDED.size, n):
            yt = torch.from_numpy(W.STRIDED[r0:r1]).to(dev)
            want = torch.from_numpy(np.ascontiguousarray(table[r0:r1, :W.n_probes(S)])).to(dev)
            lg = torch.empty(r1 - r0, S, device=dev)
            rc = lib.mvn_vnet_logits_f32(mvn._lib.ptr(yt), *[mvn._lib.ptr(t) for t in wt], mvn._lib.ptr(lg), r1 - r0, S,
                                         mvn._lib.current_stream(dev))
            assert rc == 0
            _check_logits(lg, want, yt, S, ("mvn_vnet_logits_f32", S, slow, r0))
            del lg


# ---------------------------------------------------------------- kernels without logits
FINAL_ROUTES = [({}, "vnet16_dealt_kernel<false> rings of 1"), ({"MVN_DEALT": "0", "MVN_COOP": "0"}, "vnet16_fusedn_kernel<false"),
                ({"MVN_DEALT": "8"}, "vnet16_dealt_kernel<false> rings of 8")]


@pytest.mark.parametrize("env,kernel", FINAL_ROUTES, ids=["ring1", "fusedn", "DEALT8"])
def test_sigmoid_final_metrics(oracle, dev, monkeypatch, env, kernel):
    """The 16-state kernels that write no logits, on FINAL_STRIDED as blocks of ONE symbol with final_metric_net (8 probes,
    c = +-2^-i, i = 0 ... 3), both forms: final_metric[s] = 0 - 2^40 sigmoid(c y) of probe s mod 8 bit for bit, every decision 0,
    the dealt kernels' status word 0.  (See the module docstring for what one symbol per block leaves out.)"""
    _setenv(monkeypatch, env)
    lib, S = mvn._lib.load(), 16
    y = W.FINAL_STRIDED
    table = _strided_table(oracle)[:y.size]
    nets = [_weights_t(W.final_metric_net(S, slow), dev) for slow, _ in FORMS]
    for r0, r1 in W.chunks(y.size, W.MAX_LOGIT_FLOATS // S):
        name = _kernel_name(lib, r1 - r0, 1, S, False)
        if kernel.endswith("rings of 1") and name != kernel:
            pytest.skip(f"{r1 - r0} blocks x 1 run {name!r} on this device, not the dealt kernel's rings of 1")
        assert name.startswith(kernel), name
        yt = torch.from_numpy(y[r0:r1].reshape(-1, 1).copy()).to(dev)
        want = torch.from_numpy(W.expected_final(table[r0:r1], S)).to(dev)
        for wt, (slow, _) in zip(nets, FORMS):
            dec, _, fm, nb, status = _launch(lib, dev, yt, wt, S, False)
            assert (nb > 0) == ("dealt" in kernel) and status == 0, name
            _assert_same_bits(fm, want, yt, (name, slow, r0))
            assert not bool(dec.any()), name
            del fm
