"""GPU tests (pytest -m gpu): the lock-step trial engine (trials.eval_by_word_batched) at other state counts than 16, where its block
step is mvn_vnet_byword_step_states_f32.  Every row of a batched run equals harness.eval_by_word run alone on that trial with the
separate launches (fused_step=False) and the same draws: ser_by_word, final weights, both optimizer moments and the step count
identical, as tests/test_gpu_trials.py::test_batched_trials_equal_sequential_runs asserts them at 16 states."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import states_step_cases as SC
from meta_viterbinet_amd import trials
from meta_viterbinet_amd.trials import TrialBank, TrialDraws, eval_by_word_batched
from test_gpu_reference_flow import RecordedTableDraws, _flow_kwargs, _recorded

pytestmark = pytest.mark.gpu

N_BLOCKS = 26  # one frame of 25 blocks and the pilot that starts the next


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _flow(golden, S, tag=None):
    name, selfsup = SC.FLOW[S]
    tag = tag or selfsup
    g = golden(name)
    meta = [int(v) for v in g[f"{tag}_meta"]]
    return g, tag, meta[5], meta[6]  # the golden, its tag, subframes_in_frame, nsym


def _detector(w, S, T, dev):
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w):
            p.copy_(torch.as_tensor(a).reshape(p.shape))
    return det


def _no_sequential_route(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the bank went trial after trial: the lock-step engine did not run")

    monkeypatch.setattr(trials, "_one_trial_at_a_time", refuse)


def _assert_rows_equal(bank, ser_b, seq):
    for r, (ser, wr, m, v, step) in enumerate(seq):
        assert np.array_equal(ser, ser_b[r]), (r, np.flatnonzero(ser != ser_b[r]))
        for a, b in zip(wr, bank.weights(r)):
            assert torch.equal(a, b), r
        assert torch.equal(m, bank.exp_avg[r]) and torch.equal(v, bank.exp_avg_sq[r]), r
        assert step == int(bank.step[r]), r


@pytest.mark.parametrize("S", [8, 64])
def test_lock_step_self_supervised_equals_sequential(golden, dev, monkeypatch, S):
    """R = 3 trials of the self-supervised flow (3 minibatch iterations per qualifying block) over the first 26 blocks of the
    reference's words at 8 / 64 states (L3_selfsup / L6_selfsup): the golden's words, and two copies with fresh noise on rx."""
    g, tag, sub, nsym = _flow(golden, S)
    assert sub == 25
    L, R = SC.memory(S), 3
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    tx1 = torch.tensor(g[f"{tag}_tx"][:N_BLOCKS], device=dev).float()
    rx1 = torch.tensor(g[f"{tag}_rx"][:N_BLOCKS], device=dev)
    T = rx1.shape[1]
    gen = torch.Generator(device=dev).manual_seed(64 + S)
    rx = torch.stack([rx1] + [rx1 + 0.15 * torch.randn(rx1.shape, generator=gen, device=dev) for _ in range(R - 1)]).contiguous()
    tx = tx1.unsqueeze(0).repeat(R, 1, 1).contiguous()
    kw = dict(self_supervised=True, self_supervised_iterations=3)
    seq = []
    for r in range(R):
        det = _detector(w0, S, T, dev)
        tr = mvn.OnlineTrainer(det, L)
        ser = mvn.eval_by_word(det, tx[r], rx[r], 9.0, 0.2, nsym, sub, online_trainer=tr, draws=TrialDraws(300 + r, dev),
                               fused_step=False, **kw)
        seq.append((ser, [p.detach().clone() for p in det.parameters()], tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step))
    _no_sequential_route(monkeypatch)
    bank = TrialBank([w0] * R, S, L, dev)
    rec = {}
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, [TrialDraws(300 + r, dev) for r in range(R)], record=rec, **kw)
    _assert_rows_equal(bank, ser_b, seq)
    assert rec["trained"][:, 0].all() and rec["trained"][:, 25].all()  # both pilots trained on
    assert rec["trained"].sum() > 2 * R and bank.step.min() > 0
    assert len({tuple(row) for row in ser_b}) > 1  # the trials are not copies of each other
    # the one-launch step of a lone trial (harness.eval_by_word's default at these state counts) gives the same run
    det = _detector(w0, S, T, dev)
    tr = mvn.OnlineTrainer(det, L)
    ser = mvn.eval_by_word(det, tx[1], rx[1], 9.0, 0.2, nsym, sub, online_trainer=tr, draws=TrialDraws(301, dev), **kw)
    assert np.array_equal(ser, seq[1][0]) and all(torch.equal(a, b) for a, b in zip(det.parameters(), seq[1][1]))


def test_lock_step_meta_learning_equals_sequential(golden, dev, monkeypatch):
    """The meta-learning flow at 8 states (L3_meta: an update every 5 blocks, whole-word training from the saved weights) over its first
    26 blocks with the golden's recorded draws, two identical trials."""
    S, R = 8, 2
    g, tag, sub, nsym = _flow(golden, S, "L3_meta")
    kw, opt, nsym2, sub2 = _flow_kwargs(g, None, tag, dev)
    assert (nsym2, sub2) == (nsym, sub) and not opt and kw["online_meta"]
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    tx1 = torch.tensor(g[f"{tag}_tx"][:N_BLOCKS], device=dev).float()
    rx1 = torch.tensor(g[f"{tag}_rx"][:N_BLOCKS], device=dev)
    T = rx1.shape[1]
    det = _detector(w0, S, T, dev)
    tr = mvn.OnlineTrainer(det, 3)
    last = {}

    def observer(seen):
        if seen["stage"] == "end" and seen["saved_detector"] is not None:
            last["saved"] = [p.detach().clone() for p in seen["saved_detector"].parameters()]

    ser = mvn.eval_by_word(det, tx1, rx1, 9.0, 0.2, nsym, sub, online_trainer=tr, draws=_recorded(g, tag, dev), graphed_meta=False,
                           meta_detector=mvn.META_VNETDetector(S, {"train": T, "val": T}), observer=observer, fused_step=False, **kw)
    assert np.array_equal(ser, g[f"{tag}_ser_by_word"][:N_BLOCKS])  # (the reference's own run, as far as it goes)
    seq = [(ser, [p.detach().clone() for p in det.parameters()], tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step)] * R
    _no_sequential_route(monkeypatch)
    bank = TrialBank([w0] * R, S, 3, dev)
    draws = [RecordedTableDraws(g, tag, kw["self_supervised_iterations"], sub, dev) for _ in range(R)]
    for d in draws:
        d._table = d._table[:N_BLOCKS]
    rec = {}
    ser_b = eval_by_word_batched(bank, tx1.unsqueeze(0).repeat(R, 1, 1), rx1.unsqueeze(0).repeat(R, 1, 1), nsym, sub, draws, record=rec, **kw)
    _assert_rows_equal(bank, ser_b, seq)
    assert rec["meta"].sum() >= 2 * R and rec["trained"].sum() > R
    for r in range(R):
        for a, b in zip(last["saved"], bank.weights(r, saved=True)):
            assert torch.equal(a, b), r


def test_meta_learning_at_64_states_stays_sequential(golden, dev, monkeypatch):
    """A bank at 64 states with online_meta=True (above the meta-learning kernel's 32 states) still goes trial after trial and
    returns what harness.eval_by_word returns."""
    S, N = 64, 11
    g, tag, sub, nsym = _flow(golden, S)
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    tx1 = torch.tensor(g[f"{tag}_tx"][:N], device=dev).float()
    rx1 = torch.tensor(g[f"{tag}_rx"][:N], device=dev)
    T = rx1.shape[1]
    kw = dict(online_meta=True, meta_train_iterations=1, meta_j_num=2, meta_subframes=5, MAML=False)
    det = _detector(w0, S, T, dev)
    tr = mvn.OnlineTrainer(det, 6)
    ser = mvn.eval_by_word(det, tx1, rx1, 0.0, 0.0, nsym, sub, online_trainer=tr, draws=TrialDraws(7, dev),
                           meta_detector=mvn.META_VNETDetector(S, {"train": T, "val": T}), **kw)
    calls = []
    sequential = trials._one_trial_at_a_time

    def counted(*a, **k):
        calls.append(1)
        return sequential(*a, **k)

    monkeypatch.setattr(trials, "_one_trial_at_a_time", counted)
    bank = TrialBank([w0], S, 6, dev)
    rec = {}
    ser_b = eval_by_word_batched(bank, tx1.unsqueeze(0), rx1.unsqueeze(0), nsym, sub, [TrialDraws(7, dev)], record=rec, **kw)
    assert calls == [1] and rec["meta"].any()
    _assert_rows_equal(bank, ser_b, [(ser, [p.detach().clone() for p in det.parameters()], tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step)])
