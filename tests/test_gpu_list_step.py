"""GPU tests (pytest -m gpu) of the by-word step with the reliability-ordered list decode: mvn_vnet_byword_step_list_f32 /
mvn_va_byword_step_list_f32 (byword_step.inc: byword_list_step_kernel, byword_list_step_va_kernel), mvn.list_decode and
decision='list' of harness.eval_by_word / trials.eval_by_word_batched.  Every comparison is exact (delta included: fp32 against the
referee's np.float32 arithmetic).  The expected values come from tests/list_cases.py, NumPy over the C oracle;
tests/test_list_step_host.py checks that referee and shows that the inputs make the list decoder choose other candidates."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as C
import exact_nets as X
import list_cases as Lc
import meta_viterbinet_amd as mvn
import path_cases as P
from meta_viterbinet_amd.trials import TrialBank, TrialDraws, eval_by_word_batched
from step_call import SENTINEL, step

pytestmark = pytest.mark.gpu

ALL = ("dec", "msg", "enc", "lw", "labels", "nerr", "delta", "choice")
# (T, nsym, m): 1.5 tiles; the shortest code; the reference's word with 1, 6 and 28 erasure patterns; nsym = 3 (the generator-polynomial
# encoder); 8 erasures per pattern; 63 bytes; 64 bytes (the last lane ranks a byte; whole tiles at the LDS maximum)
SHAPES = [(24, 2, 3), (16, 1, 2), (136, 2, 2), (136, 2, 4), (136, 2, 8), (136, 3, 5), (128, 8, 9), (504, 2, 4), (512, 2, 4)]


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
    """The requested outputs' rows equal the referee's, bit for bit; every padding element kept its sentinel."""
    want = {"dec": exp["dec"], "msg": exp["msg"], "nerr": exp["nerr"], "enc": exp["enc"], "lw": exp["label_word"], "labels": exp["labels"],
            "delta": exp["delta"], "choice": exp["choice"]}
    for name in names:
        if name not in out:
            continue
        flat = name in ("nerr", "choice")
        got = out[name] if flat else out[name][:, :row[name]]
        if not np.array_equal(got, want[name]):
            idx = np.argwhere(got != want[name])
            pytest.fail(f"{what}{name}{idx[0].tolist()} = {got[tuple(idx[0])]!r}, expected {want[name][tuple(idx[0])]!r}; {len(idx)} "
                        f"elements in {len(set(idx[:, 0].tolist()))} words differ")
        if not flat:
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{what}padding of {name} written"


def _priors(dev, Bp=1):
    return torch.as_tensor(np.repeat(C.channel()[1], Bp, axis=0)).to(dev).contiguous()


_EXPECTED = {}


def _case(oracle, g7w, kind, T, nsym, m, snr=6, R=64):
    """The recipe's R words at `snr` and the referee's list step on them, computed once per key."""
    key = (kind, T, nsym, m, snr, R)
    if key not in _EXPECTED:
        msg, _, y = P.words(T, nsym, R, snr)
        _EXPECTED[key] = (msg, y, Lc.expected(kind, y, msg, nsym, m, weights=g7w[0]))
    return _EXPECTED[key]


KEYS = ("dec", "delta", "choice", "msg", "nerr", "enc", "label_word", "labels")


def _rows(exp, sel):
    return {k: exp[k][sel] for k in KEYS}


def _kw(dev, g7w, kind):
    return dict(pri=_priors(dev)) if kind == "va" else dict(weights=g7w[1])


# ------------------------------------------------------------------------------------------------------------------ the data step
@pytest.mark.parametrize("R", [1, 5, 64])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym,m", SHAPES)
def test_list_step_equals_the_referee(oracle, dev, g7w, kind, T, nsym, m, R):
    msg, y, exp = _case(oracle, g7w, kind, T, nsym, m)
    if R == 64 and T >= 128:
        assert (exp["choice"] != 0).any(), "words at 6 dB: some take another candidate than the hard decoder's"
    out, row = step(dev, "list", kind, y[:R], msg[:R], nsym, m=m, **_kw(dev, g7w, kind))
    _assert_step(out, row, _rows(exp, slice(0, R)), what=f"{kind} T={T} nsym={nsym} m={m} R={R}: ")


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_list_step_on_the_host_tests_batches(oracle, dev, g7w, kind, snr):
    """The 6 and 8 dB batches whose conditions test_list_step_host.py asserts (m = 4)."""
    msg, y, exp = _case(oracle, g7w, kind, P.T_HOST, P.NSYM_HOST, 4, snr, P.R_HOST)
    out, row = step(dev, "list", kind, y, msg, P.NSYM_HOST, m=4, **_kw(dev, g7w, kind))
    _assert_step(out, row, _rows(exp, slice(None)), what=f"{kind} {snr} dB: ")


def test_vnet_list_step_with_a_weight_set_per_word(oracle, golden, dev):
    T, nsym, m, R = 136, 2, 4, 9
    msg, _, y = P.words(T, nsym, R, 6)
    base = C.g7_weights(golden)
    w = [[(a * np.float32(f)).astype(np.float32) for a in base] for f in np.linspace(0.9, 1.1, R)]
    bank = TrialBank(w, 16, C.L, dev)
    exp = [Lc.expected("vnet", y[r:r + 1], msg[r:r + 1], nsym, m, weights=w[r]) for r in range(R)]
    exp = {k: np.concatenate([e[k] for e in exp]) for k in KEYS}
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = step(dev, "list", "vnet", y, msg, nsym, m=m, weights=wp, w_stride=[bank.P] * 6)
    _assert_step(out, row, exp, what="weight set per word: ")
    assert np.any(Lc.soft(P.costs("vnet", y, w[0]))[2] != exp["delta"])  # the sets do differ


def test_va_list_step_with_a_row_of_priors_per_word(oracle, dev):
    T, nsym, m, R = 136, 2, 4, 9
    msg, _, y = P.words(T, nsym, R, 6)
    pri = (C.channel()[1] * np.linspace(0.8, 1.2, R, dtype=np.float32)[:, None]).astype(np.float32)
    exp = Lc.expected("va", y, msg, nsym, m, priors=pri)
    out, row = step(dev, "list", "va", y, msg, nsym, m=m, pri=torch.as_tensor(pri).to(dev), Bp=R)
    _assert_step(out, row, _rows(exp, slice(None)), what="priors per word: ")
    assert np.any(Lc.soft(P.costs("va", y))[2] != exp["delta"])


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym,m", [(136, 2, 4), (128, 8, 9)])
def test_list_step_honours_every_leading_dimension(oracle, dev, g7w, kind, T, nsym, m):
    msg, y, exp = _case(oracle, g7w, kind, T, nsym, m)
    K = T - 8 * nsym
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6, "delta": T + 9}
    out, row = step(dev, "list", kind, y[:5], msg[:5], nsym, m=m, ld=ld, **_kw(dev, g7w, kind))
    _assert_step(out, row, _rows(exp, slice(0, 5)), what=f"{kind} T={T} wide rows: ")


@pytest.mark.parametrize("want,with_tx", [(("nerr",), True), (("msg", "choice"), False), (("delta",), False), (("delta",), True)],
                         ids=["nerr", "no_tx:msg+choice", "no_tx:delta", "delta"])
@pytest.mark.parametrize("kind", P.KINDS)
def test_list_step_with_some_outputs_only(oracle, dev, g7w, kind, want, with_tx):
    msg, y, exp = _case(oracle, g7w, kind, 136, 2, 4)
    out, row = step(dev, "list", kind, y, msg if with_tx else None, 2, m=4, want=want, **_kw(dev, g7w, kind))
    assert sorted(out) == sorted(want)
    _assert_step(out, row, _rows(exp, slice(None)), names=want, what=f"{kind} outputs {want}: ")


@pytest.mark.parametrize("kind", P.KINDS)
def test_list_step_without_tx_refuses_outputs_that_need_it(dev, g7w, kind):
    """nerr, label_word and labels compare with the transmitted word: MVN_E_NULL without one."""
    R, T, nsym = 2, 136, 2
    rx = torch.zeros((R, T), device=dev)
    nerr = torch.zeros(R, dtype=torch.int32, device=dev)
    lib, L_ = mvn._lib.load(), mvn._lib
    tail = (None, T, None, T, None, T, None, T, None, T, L_.ptr(nerr), R, T, nsym, 0, 16, 4, None, T, None, None)
    if kind == "va":
        rc = lib.mvn_va_byword_step_list_f32(L_.ptr(rx), T, None, T, L_.ptr(_priors(dev)), 1, *tail)
    else:
        rc = lib.mvn_vnet_byword_step_list_f32(L_.ptr(rx), T, None, T, *[L_.ptr(a) for a in g7w[1]], None, *tail)
    assert rc == -4


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("T,nsym,m", [(136, 2, 4), (128, 8, 9)])
def test_pilot_step_is_the_existing_pilot_step(oracle, dev, g7w, kind, T, nsym, m):
    msg, y, _ = _case(oracle, g7w, kind, T, nsym, m)
    new, row = step(dev, "list", kind, y[:5], msg[:5], nsym, m=m, pilot=True, **_kw(dev, g7w, kind))
    old, _ = step(dev, "running", kind, y[:5], msg[:5], nsym, pilot=True, **_kw(dev, g7w, kind))
    for name in old:
        assert np.array_equal(new[name], old[name]), name
    ref = C.reference_step(None, msg[:5], nsym, True)
    assert np.array_equal(new["enc"], ref["enc"]) and np.array_equal(new["lw"], ref["enc"]) and not new["nerr"].any()
    assert np.array_equal(new["labels"], ref["labels"])
    for name in ("dec", "msg", "delta", "choice"):  # a pilot detects nothing
        assert np.all(new[name] == SENTINEL[name]), name


# ------------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("fast", [True, False], ids=["fast_sigmoid", "slow_sigmoid"])
@pytest.mark.parametrize("B,T,m", [(5, 136, 4), (70, 72, 5)])
def test_list_step_breaks_ties_towards_the_lowest_index(oracle, dev, fast, B, T, m):
    """exact_nets' staircase networks: integer logits, so delta = 0, equal byte reliabilities and equal candidate metrics abound.  delta,
    the byte order (through the candidates it selects) and the choice follow the referee's lowest-index rules."""
    c = X.tie_case(16, fast, False, B, T)
    nsym = 2
    msg = np.zeros((B, T - 8 * nsym), np.float32)
    exp = Lc.expected("vnet", c["y"], msg, nsym, m, weights=c["w"])
    assert np.array_equal(exp["dec"], c["path"])
    rho = np.abs(exp["delta"]).reshape(B, T // 8, 8).min(axis=2)
    srt = np.sort(rho, axis=1)
    assert (srt[:, m - 1] == srt[:, m]).any(), "the m-th and (m+1)-th reliabilities tie in some word: the index decides who is listed"
    Ms = np.sort(exp["metrics"], axis=1)
    if B == 70:
        assert (Ms[:, 0] == Ms[:, 1]).any(), "the minimal metric is shared in some word"
    out, row = step(dev, "list", "vnet", c["y"], msg, nsym, m=m, weights=_dev_weights(dev, c["w"]))
    _assert_step(out, row, _rows(exp, slice(None)), what=f"ties fast={fast} {B}x{T}: ")


# --------------------------------------------------------------------------------------------------------------- list_decode, flows
N_FLOW, SUB_FLOW = len(P.FLOW_ROWS), P.FLOW_SUBFRAMES
SELF_SUP = dict(self_supervised=True, self_supervised_iterations=3)
ONLINE_META = dict(self_supervised=True, self_supervised_iterations=3, online_meta=True, meta_subframes=5, meta_train_iterations=1,
                   meta_j_num=2)


def _vnet_with(w, T, dev):
    det = mvn.VNETDetector(16, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p_, a in zip(det.parameters(), w):
            p_.copy_(torch.as_tensor(a))
    return det


def _flow_words(dev):
    msg, y = P.flow_words()
    return torch.as_tensor(msg).to(dev), torch.as_tensor(y).to(dev)


@pytest.mark.parametrize("kind", P.KINDS)
def test_list_decode_is_the_step_without_a_genie(oracle, dev, g7w, kind):
    msg, y, exp = _case(oracle, g7w, kind, P.T_HOST, P.NSYM_HOST, 4, 6, P.R_HOST)
    yd = torch.as_tensor(y).to(dev)
    if kind == "va":
        det = mvn.VADetector(16, C.L, P.T_HOST, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
        got = mvn.list_decode(det, yd, P.NSYM_HOST, return_delta=True, gamma=0.2)
    else:
        got = mvn.list_decode(_vnet_with(g7w[0], P.T_HOST, dev), yd, P.NSYM_HOST, return_delta=True)
    assert np.array_equal(got[0].cpu().numpy(), exp["msg"]) and np.array_equal(got[1].cpu().numpy(), exp["choice"])
    assert np.array_equal(got[2].cpu().numpy(), exp["delta"])
    two = mvn.list_decode(det if kind == "va" else _vnet_with(g7w[0], P.T_HOST, dev), yd, P.NSYM_HOST, list_bytes=4, gamma=0.2)
    assert len(two) == 2 and torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])  # the default m is n_symbols + 2


def _run(dev, w, msg, rx, seed, decision="list", **kw):
    det = _vnet_with(w, P.T_HOST, dev)
    tr = mvn.OnlineTrainer(det, C.L)
    extra = {} if decision is None else {"decision": decision}
    ser = mvn.eval_by_word(det, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, online_trainer=tr,
                           meta_detector=mvn.META_VNETDetector(16, {"train": P.T_HOST, "val": P.T_HOST}), draws=TrialDraws(seed, dev),
                           **extra, **kw)
    return ser, [p_.detach().clone() for p_ in det.parameters()], tr


def _compose_block(det, rx_k, tx_k):
    """One data block from list_decode and the separate codec calls: (ser, the word the evaluation buffers)."""
    m_, _ = mvn.list_decode(det, rx_k, P.NSYM_HOST)
    nerr = int((m_ != tx_k).sum().item())
    enc = mvn.rs_encode(m_, P.NSYM_HOST)
    word = det.viterbi_path(rx_k) if nerr > 0 else enc
    return float(mvn.metrics.ser_from_errors(nerr, tx_k.shape[1])), word


def test_eval_by_word_list_without_updates_is_list_decode_per_block(golden, dev):
    w = C.g7_weights(golden)
    msg, rx = _flow_words(dev)
    det = _vnet_with(w, P.T_HOST, dev)
    ser = mvn.eval_by_word(det, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, decision="list")
    want = [0.0 if k % SUB_FLOW == 0 else _compose_block(det, rx[k:k + 1], msg[k:k + 1])[0] for k in range(N_FLOW)]
    assert np.array_equal(ser, np.array(want))
    ser_path = mvn.eval_by_word(det, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, decision="path")
    assert (ser > 0).sum() < (ser_path > 0).sum()  # the flow's blocks that fail under the path do not all fail under the list
    va = mvn.VADetector(16, C.L, P.T_HOST, N_FLOW, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    ser_va = mvn.eval_by_word(va, msg, rx, 8.0, 0.2, P.NSYM_HOST, SUB_FLOW, pass_count=True, decision="list")
    want_va = [0.0 if k % SUB_FLOW == 0 else
               float(mvn.metrics.ser_from_errors(int((mvn.list_decode(va, rx[k:k + 1], P.NSYM_HOST, gamma=0.2, count=k)[0] != msg[k:k + 1])
                                                     .sum().item()), msg.shape[1])) for k in range(N_FLOW)]
    assert np.array_equal(ser_va, np.array(want_va))


def test_eval_by_word_list_with_training_is_list_decode_per_block(golden, dev):
    """self_supervised: every block is checked with the weights the run had when it reached the block (snapshots taken by the observer):
    its ser and the word it buffered equal list_decode + rs_encode / viterbi_path on those weights."""
    w = C.g7_weights(golden)
    msg, rx = _flow_words(dev)
    seen = []

    def observer(s):
        if s["stage"] == "end":
            seen.append(dict(count=s["count"], ser=s["ser"], pushed=s["pushed"], word=s["buffer_tx"][-1].clone() if s["pushed"] else None,
                             w=[p_.detach().clone() for p_ in s["detector"].parameters()]))

    ser, final, tr = _run(dev, w, msg, rx, 5, observer=observer, **SELF_SUP)
    assert len(seen) == N_FLOW and tr.step > 0
    before = [torch.as_tensor(a).to(dev) for a in w]
    checked = 0
    for s in seen:
        k = s["count"]
        if k % SUB_FLOW != 0:
            det = _vnet_with([a.cpu().numpy() for a in before], P.T_HOST, dev)
            want_ser, want_word = _compose_block(det, rx[k:k + 1], msg[k:k + 1])
            assert s["ser"] == want_ser == ser[k], k
            if s["pushed"]:
                assert torch.equal(s["word"], want_word[0]), k
            checked += 1
        before = s["w"]
    assert checked == N_FLOW - N_FLOW // SUB_FLOW
    assert any(not torch.equal(p_, torch.as_tensor(o).to(dev)) for p_, o in zip(final, w))  # the run did train


def test_batched_trials_with_the_list_equal_sequential_runs(golden, dev):
    R = 3
    base = C.g7_weights(golden)
    w = [[(a * np.float32(f)).astype(np.float32) for a in base] for f in (1.0, 0.97, 1.04)]
    msg1, rx1 = _flow_words(dev)
    msg = msg1.unsqueeze(0).repeat(R, 1, 1).contiguous()
    rx = torch.stack([rx1, rx1 * 1.02, rx1 * 0.98]).contiguous()
    seq = [_run(dev, w[r], msg[r], rx[r], 100 + r, **ONLINE_META) for r in range(R)]
    bank = TrialBank(w, 16, C.L, dev)
    ser_b = eval_by_word_batched(bank, msg, rx, P.NSYM_HOST, SUB_FLOW, [TrialDraws(100 + r, dev) for r in range(R)], decision="list",
                                 **ONLINE_META)
    for r in range(R):
        assert np.array_equal(seq[r][0], ser_b[r]), r
        for p_, q_ in zip(seq[r][1], bank.weights(r)):
            assert torch.equal(p_, q_), r
        assert seq[r][2].step == int(bank.step[r]) > 0, r
    bank_m = TrialBank(w, 16, C.L, dev)
    ser_m = eval_by_word_batched(bank_m, msg, rx, P.NSYM_HOST, SUB_FLOW, [TrialDraws(100 + r, dev) for r in range(R)], decision="list",
                                 list_bytes=4, **ONLINE_META)
    assert np.array_equal(ser_m, ser_b)  # the default m is n_symbols + 2


def test_path_and_running_runs_are_unchanged_by_the_new_keyword(golden, dev):
    """decision='path' and the call without the keyword on the flow's words: the same ser and weights as the route of separate launches
    (fused_step=False), which the list step's code does not touch."""
    w = C.g7_weights(golden)
    msg, rx = _flow_words(dev)
    for decision in ("path", None, "running"):
        a, b = _run(dev, w, msg, rx, 5, decision=decision, **SELF_SUP), _run(dev, w, msg, rx, 5, decision=decision, fused_step=False, **SELF_SUP)
        assert np.array_equal(a[0], b[0]) and a[2].step == b[2].step > 0, decision
        assert all(torch.equal(p_, q_) for p_, q_ in zip(a[1], b[1])), decision
    lst = _run(dev, w, msg, rx, 5, decision="list", **SELF_SUP)
    assert not np.array_equal(lst[0], a[0])
