"""GPU tests (pytest -m gpu) of the by-word step on the traced-back Viterbi path: mvn_vnet_byword_step_path_f32 /
mvn_va_byword_step_path_f32 (byword_step.inc: byword_path_step_kernel, byword_path_step_va_kernel) and decision='path' of
harness.eval_by_word / trials.eval_by_word_batched.  Every comparison is exact.  The expected values come from the C oracle alone
(tests/path_cases.py: acs_sweep_surv + traceback, then codec_cases.reference_step); tests/test_path_step_host.py shows on the CPU that
the inputs make path and running-argmin words differ and reach every branch of the label rule."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as C
import exact_nets as X
import meta_viterbinet_amd as mvn
import path_cases as P
from meta_viterbinet_amd.trials import TrialBank, TrialDraws, eval_by_word_batched
from step_call import SENTINEL, step

pytestmark = pytest.mark.gpu

ALL = ("dec", "msg", "enc", "lw", "labels", "nerr")
LENGTHS = (24, 128, 136, 520, 1024)  # 1.5 tiles (n = 3); whole tiles; the reference's T; n = 65 (lane-stride wrap); the LDS maximum
SHAPES = [(T, nsym) for T in LENGTHS for nsym in (1, 2, 8) if nsym < T // 8]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g7w(golden, dev):
    w = C.g7_weights(golden)
    return w, [torch.as_tensor(a).to(dev).contiguous() for a in w]


def _dev_weights(dev, w):
    return [torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev).contiguous() for a in w]


def _assert_step(out, row, exp, names=ALL, what=""):
    """The requested outputs' rows equal the expected step's (exp: path_cases.expected), every padding element kept its sentinel."""
    want = {"dec": exp["dec"], "msg": exp["msg"], "nerr": exp["nerr"], "enc": exp["enc"], "lw": exp["label_word"], "labels": exp["labels"]}
    for name in names:
        if name not in out:
            continue
        got = out[name] if name == "nerr" else out[name][:, :row[name]]
        if not np.array_equal(got, want[name]):
            idx = np.argwhere(got != want[name])
            pytest.fail(f"{what}{name}{idx[0].tolist()} = {got[tuple(idx[0])]}, expected {want[name][tuple(idx[0])]}; {len(idx)} elements "
                        f"in {len(set(idx[:, 0].tolist()))} words differ")
        if name != "nerr":
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{what}padding of {name} written"


def _priors(dev, Bp=1):
    return torch.as_tensor(np.repeat(C.channel()[1], Bp, axis=0)).to(dev).contiguous()


_EXPECTED = {}


def _case(oracle, g7w, kind, T, nsym, snr=8, R=64):
    """The recipe's R words at `snr` and the expected path step on them, computed once per (kind, T, nsym, snr)."""
    key = (kind, T, nsym, snr, R)
    if key not in _EXPECTED:
        msg, _, y = P.words(T, nsym, R, snr)
        _EXPECTED[key] = (msg, y, P.expected(kind, y, msg, nsym, weights=g7w[0]))
    return _EXPECTED[key]


def _rows(exp, sel):
    return {k: (None if v is None else v[sel]) for k, v in exp.items()}


def _kw(dev, g7w, kind):
    return dict(pri=_priors(dev)) if kind == "va" else dict(weights=g7w[1])


# ------------------------------------------------------------------------------------------------------------------ the data step
@pytest.mark.parametrize("R", [1, 5, 64])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym", SHAPES)
def test_path_step_equals_the_oracle(oracle, dev, g7w, kind, T, nsym, R):
    """dec = the oracle's survivors walked back by the oracle's traceback; msg, nerr, enc, label word and trellis states = the oracle's
    step on that word.  Words at 8 dB: path and running-argmin words differ in most of them."""
    msg, y, exp = _case(oracle, g7w, kind, T, nsym)
    assert np.any(exp["dec"][:R] != exp["running"][:R]) or R == 1
    out, row = step(dev, "path", kind, y[:R], msg[:R], nsym, **_kw(dev, g7w, kind))
    _assert_step(out, row, _rows(exp, slice(0, R)), what=f"{kind} T={T} nsym={nsym} R={R}: ")


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_path_step_on_the_host_tests_batches(oracle, dev, g7w, kind, snr):
    """The exact 6 and 8 dB batches whose floors test_path_step_host.py asserts: the GPU's error counts (and everything else) equal the
    oracle's, so failed words, the 'label word = detected word' branch and decoder status 1 are reached on the GPU too."""
    msg, y, exp = _case(oracle, g7w, kind, P.T_HOST, P.NSYM_HOST, snr, P.R_HOST)
    out, row = step(dev, "path", kind, y, msg, P.NSYM_HOST, **_kw(dev, g7w, kind))
    assert np.array_equal(out["nerr"], exp["nerr"])
    _assert_step(out, row, exp, what=f"{kind} {snr} dB: ")


@pytest.mark.parametrize("kind", P.KINDS)
def test_path_step_equals_the_separate_launches(oracle, dev, g7w, kind):
    """One launch against the library's own route: viterbi_path (sweep with survivors + traceback), rs_decode, a plain comparison,
    rs_encode, calculate_states."""
    T, nsym = 136, 2
    msg, y, _ = _case(oracle, g7w, kind, T, nsym)
    yd, md = torch.as_tensor(y).to(dev), torch.as_tensor(msg).to(dev)
    if kind == "va":
        det = mvn.VADetector(16, C.L, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
        dec = det.viterbi_path(yd, 8.0, 0.2)
    else:
        det = mvn.VNETDetector(16, {"train": T, "val": T}).to(dev)
        with torch.no_grad():
            for p_, a in zip(det.parameters(), g7w[0]):
                p_.copy_(torch.as_tensor(a))
        dec = det.viterbi_path(yd)
    dmsg = mvn.rs_decode(dec, nsym)
    enc = mvn.rs_encode(dmsg, nsym)
    nerr = (dmsg != md).sum(dim=1).to(torch.int32)
    lw = torch.where((nerr > 0).reshape(-1, 1), dec, enc)
    lib_route = dict(dec=dec.cpu().numpy(), msg=dmsg.cpu().numpy(), nerr=nerr.cpu().numpy(), enc=enc.cpu().numpy(),
                     label_word=lw.cpu().numpy(), labels=mvn.calculate_states(C.L, lw).reshape(lw.shape).to(torch.int32).cpu().numpy())
    out, row = step(dev, "path", kind, y, msg, nsym, **_kw(dev, g7w, kind))
    _assert_step(out, row, lib_route, what=f"{kind} against the separate launches: ")
    assert (lib_route["nerr"] > 0).any() and (lib_route["nerr"] == 0).any()


def test_vnet_path_step_with_a_weight_set_per_word(oracle, golden, dev):
    """R weight sets through w_stride (a TrialBank's rows): word r is detected with set r."""
    T, nsym, R = 136, 2, 9
    msg, _, y = P.words(T, nsym, R, 8)
    base = C.g7_weights(golden)
    w = [[(a * np.float32(f)).astype(np.float32) for a in base] for f in np.linspace(0.9, 1.1, R)]
    bank = TrialBank(w, 16, C.L, dev)
    exp = [P.expected("vnet", y[r:r + 1], msg[r:r + 1], nsym, weights=w[r]) for r in range(R)]
    exp = {k: np.concatenate([e[k] for e in exp]) for k in ("dec", "msg", "nerr", "enc", "label_word", "labels")}
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = step(dev, "path", "vnet", y, msg, nsym, weights=wp, w_stride=[bank.P] * 6)
    _assert_step(out, row, exp, what="weight set per word: ")
    shared = P.expected("vnet", y, msg, nsym, weights=w[0])
    assert np.any(shared["dec"] != exp["dec"])  # the sets do decide differently


def test_va_path_step_with_a_row_of_priors_per_word(oracle, dev):
    """Bp = R rows of state priors, each word its own: the channel scaled by 0.5 .. 1.5, far enough off at both ends that the oracle
    decides those words differently than with the true channel."""
    T, nsym, R = 136, 2, 9
    msg, _, y = P.words(T, nsym, R, 8)
    pri = (C.channel()[1] * np.linspace(0.5, 1.5, R, dtype=np.float32)[:, None]).astype(np.float32)
    exp = P.expected("va", y, msg, nsym, priors=pri)
    out, row = step(dev, "path", "va", y, msg, nsym, pri=torch.as_tensor(pri).to(dev), Bp=R)
    _assert_step(out, row, exp, what="priors per word: ")
    assert np.any(P.expected("va", y, msg, nsym)["dec"] != exp["dec"])


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym", [(136, 2), (520, 8)])
def test_path_step_honours_every_leading_dimension(oracle, dev, g7w, kind, T, nsym):
    msg, y, exp = _case(oracle, g7w, kind, T, nsym)
    K = T - 8 * nsym
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6}
    out, row = step(dev, "path", kind, y[:5], msg[:5], nsym, ld=ld, **_kw(dev, g7w, kind))
    _assert_step(out, row, _rows(exp, slice(0, 5)), what=f"{kind} T={T} wide rows: ")


@pytest.mark.parametrize("want", [("nerr",), ("dec", "nerr"), ("lw", "labels")], ids=["nerr", "dec+nerr", "lw+labels"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_path_step_with_some_outputs_only(oracle, dev, g7w, kind, want):
    msg, y, exp = _case(oracle, g7w, kind, 136, 2)
    out, row = step(dev, "path", kind, y, msg, 2, want=want, **_kw(dev, g7w, kind))
    assert sorted(out) == sorted(want)
    _assert_step(out, row, exp, names=want, what=f"{kind} outputs {want}: ")


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym", [(136, 2), (128, 8)])
def test_pilot_step_is_the_existing_pilot_step(oracle, dev, g7w, kind, T, nsym):
    msg, y, _ = _case(oracle, g7w, kind, T, nsym)
    new, row = step(dev, "path", kind, y[:5], msg[:5], nsym, pilot=True, **_kw(dev, g7w, kind))
    old, _ = step(dev, "running", kind, y[:5], msg[:5], nsym, pilot=True, **_kw(dev, g7w, kind))
    for name in ALL:
        assert np.array_equal(new[name], old[name]), name
    ref = C.reference_step(None, msg[:5], nsym, True)
    assert np.array_equal(new["enc"], ref["enc"]) and np.array_equal(new["lw"], ref["enc"]) and not new["nerr"].any()
    assert np.array_equal(new["labels"], ref["labels"])
    assert np.all(new["dec"] == SENTINEL["dec"]) and np.all(new["msg"] == SENTINEL["msg"])


# -------------------------------------------------------------------------------------------------------- ties, non-finite values
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("fast", [True, False], ids=["fast_sigmoid", "slow_sigmoid"])
@pytest.mark.parametrize("B,T", [(5, 136), (3, 200), (70, 72)])
def test_path_step_breaks_ties_like_torch(oracle, dev, fast, strict, B, T):
    """exact_nets' staircase networks: survivor choices tie at several per cent of the stages, and some final metrics tie at the
    minimum.  dec equals the NumPy textbook path, the oracle's and VNETDetector.viterbi_path's; the walk starts at the first index."""
    c = X.tie_case(16, fast, strict, B, T)
    nsym = 2
    msg = np.zeros((B, T - 8 * nsym), np.float32)
    exp = P.expected("vnet", c["y"], msg, nsym, weights=c["w"])
    assert np.array_equal(exp["dec"], c["path"])  # the oracle agrees with the NumPy reference
    wd = _dev_weights(dev, c["w"])
    out, row = step(dev, "path", "vnet", c["y"], msg, nsym, weights=wd)
    _assert_step(out, row, exp, what=f"ties fast={fast} strict={strict} {B}x{T}: ")
    det = mvn.VNETDetector(16, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p_, a in zip(det.parameters(), c["w"]):
            p_.copy_(torch.as_tensor(a))
    assert np.array_equal(det.viterbi_path(torch.as_tensor(c["y"]).to(dev)).cpu().numpy(), out["dec"])


def test_vnet_path_step_with_partially_nan_costs(oracle, golden, dev):
    """A NaN and a 1e30 entry in W3: some of a symbol's branch costs are NaN, the strict (torch.min) form of the sweep runs, survivors
    take the first NaN's index."""
    T, nsym, R = 136, 2, 9
    msg, _, y = P.words(T, nsym, R, 8)
    w = [a.copy() for a in C.g7_weights(golden)]
    w[4][3, 11] = np.nan
    w[4][9, 2] = 1e30
    exp = P.expected("vnet", y, msg, nsym, weights=w)
    out, row = step(dev, "path", "vnet", y, msg, nsym, weights=_dev_weights(dev, w))
    _assert_step(out, row, exp, what="NaN / 1e30 in W3: ")


@pytest.mark.parametrize("kind", P.KINDS)
def test_path_step_with_infinite_samples(oracle, dev, g7w, kind):
    T, nsym, R = 136, 2, 6
    msg, _, y = P.words(T, nsym, R, 8)
    y = y.copy()
    y[1, 40], y[2, 0], y[3, 135], y[4, 77] = np.inf, -np.inf, np.inf, -np.inf
    exp = P.expected(kind, y, msg, nsym, weights=g7w[0])
    out, row = step(dev, "path", kind, y, msg, nsym, **_kw(dev, g7w, kind))
    _assert_step(out, row, exp, what=f"{kind} +-inf samples: ")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_va_path_step_with_a_non_finite_prior(oracle, dev, bad):
    T, nsym, R = 136, 2, 6
    msg, _, y = P.words(T, nsym, R, 8)
    pri = C.channel()[1].copy()
    pri[0, 9] = bad
    exp = P.expected("va", y, msg, nsym, priors=pri)
    out, row = step(dev, "path", "va", y, msg, nsym, pri=torch.as_tensor(pri).to(dev))
    _assert_step(out, row, exp, what=f"prior {bad}: ")


# --------------------------------------------------------------------------------------------------------------------------- flows
N_FLOW, SUB_FLOW = len(P.FLOW_ROWS), P.FLOW_SUBFRAMES
FLOWS = {
    "self_supervised": dict(self_supervised=True, self_supervised_iterations=3),
    "online_meta": dict(self_supervised=True, self_supervised_iterations=3, online_meta=True, meta_subframes=5, meta_train_iterations=1,
                        meta_j_num=2),
}


def _vnet_with(w, T, dev):
    det = mvn.VNETDetector(16, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p_, a in zip(det.parameters(), w):
            p_.copy_(torch.as_tensor(a))
    return det


def _flow_words(dev):
    msg, y = P.flow_words()
    return torch.as_tensor(msg).to(dev), torch.as_tensor(y).to(dev)


def _run(dev, w, msg, rx, seed, decision="path", fused=True, **kw):
    det = _vnet_with(w, P.T_HOST, dev)
    tr = mvn.OnlineTrainer(det, C.L)
    extra = {} if decision is None else {"decision": decision}
    ser = mvn.eval_by_word(det, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, online_trainer=tr,
                           meta_detector=mvn.META_VNETDetector(16, {"train": P.T_HOST, "val": P.T_HOST}), draws=TrialDraws(seed, dev),
                           fused_step=fused, **extra, **kw)
    return ser, [p_.detach().clone() for p_ in det.parameters()], tr


@pytest.mark.parametrize("flow", sorted(FLOWS))
def test_eval_by_word_on_the_path_fused_equals_separate_launches(golden, dev, flow):
    w = C.g7_weights(golden)
    msg, rx = _flow_words(dev)
    a, b = _run(dev, w, msg, rx, 5, fused=True, **FLOWS[flow]), _run(dev, w, msg, rx, 5, fused=False, **FLOWS[flow])
    assert np.array_equal(a[0], b[0]) and a[2].step == b[2].step > 0
    for p_, q_ in zip(a[1], b[1]):
        assert torch.equal(p_, q_)
    assert any(not torch.equal(p_, torch.as_tensor(o).to(dev)) for p_, o in zip(a[1], w))  # the run did train
    # without updates: the error counts alone
    plain = [mvn.eval_by_word(_vnet_with(w, P.T_HOST, dev), msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, fused_step=f, decision="path")
             for f in (True, False)]
    assert np.array_equal(plain[0], plain[1])


def test_eval_by_word_on_the_path_va_with_the_block_number(dev):
    msg, rx = _flow_words(dev)
    det = mvn.VADetector(16, C.L, P.T_HOST, N_FLOW, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    sers = [mvn.eval_by_word(det, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, pass_count=True, fused_step=f, decision="path") for f in (True, False)]
    assert np.array_equal(sers[0], sers[1])
    _, path = P.detect(P.costs("va", rx.cpu().numpy()))
    ref = C.reference_step(path, msg.cpu().numpy(), P.NSYM_HOST, False)["nerr"]
    data = np.arange(N_FLOW) % SUB_FLOW != 0
    assert np.array_equal(sers[0][data] > 0, ref[data] > 0) and not sers[0][~data].any()


def test_running_decision_is_the_call_without_the_keyword(golden, dev):
    w = C.g7_weights(golden)
    msg, rx = _flow_words(dev)
    a, b = _run(dev, w, msg, rx, 5, decision="running", **FLOWS["self_supervised"]), _run(dev, w, msg, rx, 5, decision=None, **FLOWS["self_supervised"])
    assert np.array_equal(a[0], b[0]) and all(torch.equal(p_, q_) for p_, q_ in zip(a[1], b[1]))
    c = _run(dev, w, msg, rx, 5, decision="path", **FLOWS["self_supervised"])
    assert not np.array_equal(a[0], c[0])  # (at 8 dB the two rules do not fail on the same words)


def test_batched_trials_on_the_path_equal_sequential_runs(golden, dev):
    R = 3
    base = C.g7_weights(golden)
    w = [[(a * np.float32(f)).astype(np.float32) for a in base] for f in (1.0, 0.97, 1.04)]
    msg1, rx1 = _flow_words(dev)
    msg = msg1.unsqueeze(0).repeat(R, 1, 1).contiguous()
    rx = torch.stack([rx1, rx1 * 1.02, rx1 * 0.98]).contiguous()
    kw = FLOWS["online_meta"]
    seq = [_run(dev, w[r], msg[r], rx[r], 100 + r, **kw) for r in range(R)]
    bank = TrialBank(w, 16, C.L, dev)
    ser_b = eval_by_word_batched(bank, msg, rx, P.NSYM_HOST, SUB_FLOW, [TrialDraws(100 + r, dev) for r in range(R)], decision="path", **kw)
    for r in range(R):
        assert np.array_equal(seq[r][0], ser_b[r]), r
        for p_, q_ in zip(seq[r][1], bank.weights(r)):
            assert torch.equal(p_, q_), r
        assert seq[r][2].step == int(bank.step[r]) > 0, r
    bank_run = TrialBank(w, 16, C.L, dev)
    ser_run = eval_by_word_batched(bank_run, msg, rx, P.NSYM_HOST, SUB_FLOW, [TrialDraws(100 + r, dev) for r in range(R)], **kw)
    assert not np.array_equal(ser_run, ser_b)
