"""GPU tests (pytest -m gpu) of the two data-dependent choices of the ViterbiNet kernels that random-normal inputs reach at symbol 0
only: which of two EQUAL path metrics wins (torch.min / torch.argmin: the first index), and which sigmoid form a tile takes and
what happens just past the switch.  Inputs and references come from tests/exact_nets.py (test_exact_nets_host.py checks them on
the CPU): the tie tests compare with a float64 MLP + a NumPy textbook Viterbi, the sigmoid-range tests with the C oracle.  Every
comparison is bit for bit.

What the tie tests were seen to catch (edits tried on a scratch build, never committed).  (1) decide_lsb / decide_lsb_strict
(vnet16_common.inc) letting the LAST minimal index win unless the minimum is 0, and the dealt kernel's survivor store taking
`pa <= a`: every 16-state case of test_vnet_routes_*, all of test_vnet16_dealt_*, test_byword_step_*, test_viterbi_path_* and the
fused (70 x 72, 16 states) cases of test_vnet_survivors_* fail; of the ViterbiNet tests on random weights only three very large
shapes notice, through a chance tie (and the inf / NaN tests, whose non-finite metrics tie).  (The same edit without the
exception for 0 is caught by any test at symbol 0, where all metrics are 0.)  (2) va_ip_decide_u / va_ip_decide_strict_u (va_inplace.inc) letting a lane's last tied slot win unless the
minimum is 0: the MVN_FUSED_IP=1 cases at 4, 8, 32 and 128 states fail, where test_vnet_fused_ip_and_two_kernel_routes and
test_vnet_vs_oracle pass (the sweeps and the VA kernels, which share that function, have tie inputs of their own and notice)."""
import ctypes

import numpy as np
import pytest
import torch

import exact_nets as E
import meta_viterbinet_amd as mvn
from test_gpu_parity import VNET_NAN_ROUTES, _dealt_call, _np, _vnet_with, _weights_t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


# VNET_NAN_ROUTES hands every call a workspace, with which MVN_COOP=0 alone runs the dealt kernel on rings of 8: the
# one-wave-per-block kernel at its default super-tile is pinned as a route of its own here
ROUTES = VNET_NAN_ROUTES + [(16, {"MVN_COOP": "0", "MVN_DEALT": "0"})]
ROUTE_IDS = [f"S{s}-" + "-".join(f"{k[4:]}{v}" for k, v in e.items()) for s, e in ROUTES]
# (B, T, switches) that run vnet16_dealt_kernel: one block per ring of 8; fewer blocks than wave slots; every ring size; blocks that
# cross group boundaries
DEALT_CASES = [(3, 200, {"MVN_COOP": "0"}), (801, 31, {}), (7000, 40, {"MVN_DEALT": "8"}), (7000, 40, {"MVN_DEALT": "4"}),
               (7000, 40, {"MVN_DEALT": "2"}), (7000, 40, {}), (1100, 72, {})]
DEALT_IDS = [f"{b}x{t}" + "".join(f"-{k[4:]}{v}" for k, v in e.items()) for b, t, e in DEALT_CASES]
FORMS = pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
STRICT = pytest.mark.parametrize("strict", [False, True], ids=["minnum", "strict"])


def _kernel_name(lib, B, T, S, want_logits=False):
    name = ctypes.create_string_buffer(96)
    assert lib.mvn_vnet_decode_kernel_name(B, T, S, 1 if want_logits else 0, name, 96) == 0
    return name.value.decode()


def _decode(lib, dev, yt, wt, S, want_logits):
    """mvn_vnet_decode_f32 as test_vnet_partial_nan_follows_torch_min calls it (a workspace that holds the batch's logits)."""
    B, T = yt.shape
    dec, fm = torch.full((B, T), 7.0, device=dev), torch.empty(B, S, device=dev)
    lg = torch.empty(B, T, S, device=dev) if want_logits else None
    ws = torch.empty(B * T * S * 4, dtype=torch.uint8, device=dev)
    rc = lib.mvn_vnet_decode_f32(mvn._lib.ptr(yt), T, *[mvn._lib.ptr(t) for t in wt], mvn._lib.ptr(dec), T, mvn._lib.ptr(lg),
                                 mvn._lib.ptr(fm), mvn._lib.ptr(ws), ws.numel(), B, T, S, mvn._lib.current_stream(dev))
    assert rc == 0
    return dec, lg, fm


def _check_route(lib, dev, S, y, w, rdec, rlg, rfm, dealt=False):
    """Decisions, final metrics and (second call) logits of one route against a reference."""
    B, T = y.shape
    yt, wt = torch.tensor(y, device=dev), _weights_t(w, dev)
    for want_logits in (False, True):
        what = (_kernel_name(lib, B, T, S, want_logits), B, T)
        if dealt:
            assert what[0].startswith(f"vnet16_dealt_kernel<{'true' if want_logits else 'false'}> rings of "), what
            dec, lg, fm, ws, nb = _dealt_call(lib, dev, yt, wt, B, T, want_logits=want_logits)
            assert nb > 0 and int(ws[:4].view(torch.int32).item()) == 0, what  # no hand-off was abandoned
        else:
            dec, lg, fm = _decode(lib, dev, yt, wt, S, want_logits)
        assert np.array_equal(_np(dec), rdec), what
        assert np.array_equal(_np(fm), rfm), what
        if want_logits:
            assert np.array_equal(_np(lg), rlg), what


def _numpy_count(dec, tx, rows):
    err = dec[rows][:, :tx.shape[1]] != tx[rows]
    return [int(err.sum()), int(err.size), int(err.any(axis=1).sum()), len(rows)]


# ---------------------------------------------------------------- exact ties
@pytest.mark.parametrize("S,env", ROUTES, ids=ROUTE_IDS)
@FORMS
@STRICT
def test_vnet_routes_break_ties_like_torch(dev, monkeypatch, S, env, fast, strict):
    """Every route of mvn_vnet_decode_f32 on the staircase networks, whose path metrics tie at 1-7 % of the decisions and survivor
    choices after symbol 0: decisions, final metrics and logits are those of ideal_logits + textbook_acs (first index wins), with
    the fast and the slow sigmoid, and with one weight past kStrictMinBound (the strict stage and decision, the guard launch)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = mvn._lib.load()
    for B, T in E.TIE_SHAPES[S][:2]:  # (9, 75), (5, 33)
        c = E.tie_case(S, fast, strict, B, T)
        _check_route(lib, dev, S, c["y"], c["w"], c["dec"], c["logits"], c["fm"])


@pytest.mark.parametrize("B,T,env", DEALT_CASES, ids=DEALT_IDS)
@FORMS
@STRICT
def test_vnet16_dealt_breaks_ties_like_torch(dev, monkeypatch, B, T, env, fast, strict):
    """vnet16_dealt_kernel (the headline's default route) on the staircase networks: decisions, logits and final metrics across
    unit, ring and group boundaries, and the four counters of mvn_vnet_decode_count_f32 against a plain NumPy count."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = mvn._lib.load()
    c = E.tie_case(16, fast, strict, B, T)
    _check_route(lib, dev, 16, c["y"], c["w"], c["dec"], c["logits"], c["fm"], dealt=True)
    rng = np.random.RandomState(B + T)
    K = max(1, T - 5)
    tx = np.where(rng.rand(B, K) < 0.9, c["dec"][:, :K], 1.0 - c["dec"][:, :K]).astype(np.float32)  # a tenth of the bits in error
    rows = np.array([i for i in range(B) if i % 5 != 0], np.int64)
    mask = torch.zeros(B, dtype=torch.uint8, device=dev)
    mask[torch.tensor(rows, device=dev)] = 1
    dec, cnt, _, _ = _dealt_call(lib, dev, torch.tensor(c["y"], device=dev), _weights_t(c["w"], dev), B, T,
                                 tx=torch.tensor(tx, device=dev), K=K, mask=mask)
    assert np.array_equal(_np(dec), c["dec"])
    assert cnt.tolist() == _numpy_count(c["dec"], tx, rows)


@pytest.mark.parametrize("S", [4, 16, 64])
@pytest.mark.parametrize("B,T", [(5, 33), (70, 72)])
@FORMS
@STRICT
def test_vnet_survivors_break_ties_like_torch(dev, S, B, T, fast, strict):
    """mvn_vnet_decode_surv_f32: the survivor bit of a tied state is torch.min's index 0; bytes and the traced-back path against the
    textbook Viterbi.  16 states at T % 4 == 0: vnet16_dealt_kernel<false, true> stores them itself; else the two-kernel route."""
    c = E.tie_case(S, fast, strict, B, T)
    lib, st = mvn._lib.load(), mvn._lib.current_stream(dev)
    yt, wt = torch.tensor(c["y"], device=dev), _weights_t(c["w"], dev)
    dec, fm = torch.full((B, T), 7.0, device=dev), torch.empty(B, S, device=dev)
    surv = torch.full((B, T, max(1, S // 8)), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(int(lib.mvn_vnet_surv_workspace_bytes(B, T, S)), 16), dtype=torch.uint8, device=dev)
    rc = lib.mvn_vnet_decode_surv_f32(mvn._lib.ptr(yt), T, *[mvn._lib.ptr(t) for t in wt], mvn._lib.ptr(dec), T, mvn._lib.ptr(fm),
                                      mvn._lib.ptr(surv), mvn._lib.ptr(ws), ws.numel(), B, T, S, st)
    assert rc == 0
    assert np.array_equal(_np(dec), c["dec"]) and np.array_equal(_np(fm), c["fm"])
    got = _np(surv)
    diff = np.argwhere(got != c["surv"])
    assert diff.size == 0, (len(diff), diff[:4].tolist())
    bits, states = mvn.traceback(surv, fm, return_states=True)
    assert np.array_equal(_np(bits), c["path"]) and np.array_equal(_np(states) & 1, c["path"].astype(np.int64))


@FORMS
@STRICT
def test_byword_step_breaks_ties_like_torch(dev, fast, strict):
    """mvn_vnet_byword_step_f32 (a 16-wave workgroup per word): its `dec` output for R = 5 words of K = 120 message bits + 2 parity
    bytes on the staircase grid (the words need not be codewords: the RS outputs are tested elsewhere)."""
    R, K, nsym = 5, 120, 2
    T = K + 8 * nsym
    c = E.tie_case(16, fast, strict, R, T)
    rx, wt = torch.tensor(c["y"], device=dev), _weights_t(c["w"], dev)
    tx = torch.tensor(c["dec"][:, :K].copy(), device=dev)
    dec = torch.full((R, T), 7.0, device=dev)
    rc = mvn._lib.load().mvn_vnet_byword_step_f32(mvn._lib.ptr(rx), T, mvn._lib.ptr(tx), K, *[mvn._lib.ptr(t) for t in wt], None,
                                                  mvn._lib.ptr(dec), T, None, K, None, T, None, T, None, T, None, R, T, nsym, 0, 16,
                                                  mvn._lib.current_stream(dev))
    assert rc == 0
    assert np.array_equal(_np(dec), c["dec"])


def test_viterbi_path_breaks_ties_like_torch(dev):
    """VNETDetector.viterbi_path end to end on one staircase case: the textbook path, decisions, metrics and survivors."""
    S, B, T = 16, 70, 72
    c = E.tie_case(S, False, False, B, T)
    det = _vnet_with(c["w"], S, T, dev)
    bits, dec, fm, surv = det.viterbi_path(torch.tensor(c["y"], device=dev), return_all=True)
    assert np.array_equal(_np(bits), c["path"]) and np.array_equal(_np(dec), c["dec"])
    assert np.array_equal(_np(fm), c["fm"]) and np.array_equal(_np(surv), c["surv"])


# ---------------------------------------------------------------- sigmoid range and the subnormal pin
# (S, switches, [(B, T)], the dealt kernel's call): the 16-state routes, the dealt kernel on rings of 8 and by default,
# vnet_fused_ip_kernel<LB>, the two-kernel route
SIGMOID_ROUTES = [(S, e, [(9, 75), (5, 33)], False) for S, e in ROUTES if S == 16] + \
                 [(16, {"MVN_COOP": "0"}, [(3, 200)], True), (16, {}, [(801, 31)], True)] + \
                 [(S, {"MVN_FUSED_IP": "1"}, [(9, 75), (5, 33)], False) for S in (4, 32, 128)] + \
                 [(S, {"MVN_UNFUSED": "1"}, [(9, 75), (5, 33)], False) for S in (8, 256)]
SIGMOID_IDS = [f"S{s}-" + "-".join(f"{k[4:]}{v}" for k, v in e.items()) + ("-dealt" if d else "")
               for s, e, _, d in SIGMOID_ROUTES]


@pytest.mark.parametrize("S,env,shapes,dealt", SIGMOID_ROUTES, ids=SIGMOID_IDS)
def test_vnet_sigmoid_range_ladder(oracle, dev, monkeypatch, S, env, shapes, dealt):
    """Samples that put a tile's bound max|y| max|W1| + max|b1| on 85.9, 86.0 (the last value of the fast form), 86.1, into the
    range where the sigmoid is a subnormal float (87.5, 88.5), past exp's clamps (95, 104.5, 130) and up to 1e6 and 3e38, with either
    sign, next to -0.0 and a subnormal sample; slow tiles between fast ones and inside a tile of ordinary samples.  Decisions, logits
    and final metrics are the oracle's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = mvn._lib.load()
    w = E.ladder_weights(S, np.random.RandomState(S))
    for B, T in shapes:
        y = E.ladder_samples(B, T, np.random.RandomState(S + B + T))
        rdec, rlg, rfm = oracle.vnet_decode(y, w, want_logits=True, want_final=True)
        assert np.isfinite(rlg).all()
        _check_route(lib, dev, S, y, w, rdec, rlg, rfm, dealt=dealt)


@pytest.mark.parametrize("S,env,shapes,dealt", SIGMOID_ROUTES, ids=SIGMOID_IDS)
@pytest.mark.parametrize("k,j", E.SUBNORMAL_KJ)
def test_vnet_subnormal_activation_is_kept(oracle, dev, monkeypatch, S, env, shapes, dealt, k, j):
    """One subnormal hidden-1 activation (sigmoid(-88) = 6.05e-39, unit k) alone decides half of the logits through hidden-2 unit j
    -- a row of the MFMA operands (j = 5, 47) or one of the two fmaf-chain units (48, 49) -- and the decisions of the all-1.0
    block: logits and decisions are the oracle's (which test_exact_nets_host.py shows to differ from a flushed activation's)."""
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    lib = mvn._lib.load()
    B, T = shapes[0]
    w = E.subnormal_net(S, k, j, np.random.RandomState(100 * k + j))
    y = E.subnormal_samples(B, T, np.random.RandomState(k + j))
    rdec, rlg, rfm = oracle.vnet_decode(y, w, want_logits=True, want_final=True)
    half = (np.arange(S) & 2) != 0
    assert np.all(rlg[0][:, half] == np.float32(6.054601e-39) * np.float32(2.0 ** 80)) and np.all(rdec[0, 1:] == 1.0)
    _check_route(lib, dev, S, y, w, rdec, rlg, rfm, dealt=dealt)
