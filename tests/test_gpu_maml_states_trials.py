"""GPU tests (pytest -m gpu): the trial axis of the meta-learning step at 64 and 128 states -- mvn_vnet_maml_train_states_trials_f32
(maml_train_states_trials_kernel<64 | 128>, one workgroup per trial, grid (1, R)) and the lock-step engine that launches it
(trials.eval_by_word_batched with online_meta at 64 / 128 states).

The kernel runs the body of the one-trial kernel, so every trial of a launch must give the bits of mvn_vnet_maml_train_ws_f32 run
alone on copies of its arrays: torch.equal throughout, no tolerance.  Inputs as in test_gpu_maml_states.py: G17's weights, G21's
received words, labels from random bits through calculate_states.  The engine's rows are compared, bit for bit, with
harness.eval_by_word run alone on each trial with the same draws, and row 0 of a full G21 run with the reference's recording."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import test_gpu_reference_flow as RF
from meta_viterbinet_amd import _lib, trials
from meta_viterbinet_amd.trials import TRIAL_DTYPE, TrialBank, TrialDraws, beta_power, eval_by_word_batched, param_offsets
from test_gpu_maml_states import STATES, _inputs, _vnet_with

pytestmark = pytest.mark.gpu

META_LR, LR, B1, B2, EPS = 0.1, 1e-3, 0.9, 0.999, 1e-8
SENTINEL = 777.25
G21_WEIGHT_TOL = 5e-5  # test_gpu_maml_states.py::test_reference_meta_flow_64_128_states's bound on |w - the reference's|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the entry point, by hand
def _six(row, S):
    """device addresses of W1, b1, W2, b2, W3, b3 inside a flat parameter row"""
    off = param_offsets(S)
    return [row.data_ptr() + 4 * int(off[a]) for a in range(6)]


def _steps(n, W, shift, dev):
    """support words [n, W] and query word [n] of a trial's steps among the 10 buffered words (another set per `shift`)"""
    sup = np.array([[(shift + k + j) % 10 for j in range(W)] for k in range(max(n, 1))], np.int32)
    qry = np.array([(shift + k + W) % 10 for k in range(max(n, 1))], np.int32)
    return torch.tensor(sup, device=dev), torch.tensor(qry, device=dev)


def _alone(lib, dev, S, T, W, second, rx, lab, sup, qry, n, start, m, v, step0):
    """mvn_vnet_maml_train_ws_f32 on copies: (weights, exp_avg, exp_avg_sq) after n steps from `start`"""
    th, m, v = start.clone(), m.clone(), v.clone()
    with torch.cuda.device(dev):
        rc = lib.mvn_vnet_maml_train_ws_f32(_lib.ptr(rx), _lib.ptr(lab), T, _lib.ptr(sup), W, _lib.ptr(qry), n,
                                            *[ctypes.c_void_p(p) for p in _six(th, S)], _lib.ptr(m), _lib.ptr(v), step0, META_LR,
                                            second, LR, B1, B2, EPS, None, S, None, 0, None, _lib.current_stream(dev))
    _lib.check(rc, "mvn_vnet_maml_train_ws_f32")
    torch.cuda.synchronize(dev)
    return th, m, v


def _launch(lib, dev, desc, T, W, second, S):
    d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    with torch.cuda.device(dev):
        rc = lib.mvn_vnet_maml_train_states_trials_f32(_lib.ptr(d), len(desc), T, W, META_LR, second, LR, B1, B2, EPS, S,
                                                       _lib.current_stream(dev))
    _lib.check(rc, "mvn_vnet_maml_train_states_trials_f32")
    torch.cuda.synchronize(dev)  # (d lives until here)


def _describe(d, rx, lab, sup, qry, w_in, w_out, w_out2, m, v, step0, n, S):
    d["y"], d["labels"], d["idx"], d["query_idx"] = rx.data_ptr(), lab.data_ptr(), sup.data_ptr(), qry.data_ptr()
    d["w_in"], d["w_out"] = _six(w_in, S), _six(w_out, S)
    d["w_out2"] = _six(w_out2, S) if w_out2 is not None else 0
    d["adam_m"], d["adam_v"], d["loss_out"], d["status"] = m.data_ptr(), v.data_ptr(), 0, 0
    d["b1pow"], d["b2pow"] = beta_power(B1, step0), beta_power(B2, step0)
    d["n"], d["reserved"] = n, 0


def _four_trials(lib, dev, S, T, W, second):
    """The four hand-filled trials of one launch: the state before, the state after, and what the one-trial call gives for each."""
    w, rx, _, labels = _inputs(S, T)
    rxd, labd = torch.tensor(rx, device=dev), torch.tensor(labels.astype(np.int32), device=dev)
    base = torch.cat([torch.as_tensor(a).reshape(-1) for a in w]).to(dev)
    P = base.numel()
    assert P == int(param_offsets(S)[-1])
    gen = torch.Generator(device=dev).manual_seed(1000 + S + T)

    def near(rows):
        return (base + 0.01 * torch.randn((rows, P), generator=gen, device=dev)).contiguous()

    theta, saved, shared = near(4), near(4), near(1)[0].contiguous()
    m = (1e-3 * torch.randn((4, P), generator=gen, device=dev)).contiguous()
    v = torch.empty((4, P), device=dev).uniform_(1e-7, 1e-5, generator=gen)
    for t in (theta, saved, m, v):
        t[1] = SENTINEL  # trial 1 does nothing
    # (n, step0, w_in, w_out, w_out2)
    spec = [(3, 0, theta[0], theta[0], None),         # training in place, no second copy, zero steps behind it
            (0, 5, saved[1], theta[1], saved[1]),     # skipped
            (2, 1023, saved[2], theta[2], saved[2]),  # restart from the saved row (the engine's last_frame), b1pow / b2pow != 1
            (1, 7, shared, theta[3], saved[3])]       # start from a row that is nobody's output
    steps = [_steps(n, W, 3 * r, dev) for r, (n, *_) in enumerate(spec)]
    before = dict(theta=theta.clone(), saved=saved.clone(), m=m.clone(), v=v.clone(), shared=shared.clone())
    alone = [None if n == 0 else _alone(lib, dev, S, T, W, second, rxd, labd, *steps[r], n, w_in, m[r], v[r], step0)
             for r, (n, step0, w_in, _, _) in enumerate(spec)]
    desc = np.zeros(4, TRIAL_DTYPE)
    for r, (n, step0, w_in, w_out, w_out2) in enumerate(spec):
        _describe(desc[r:r + 1], rxd, labd, *steps[r], w_in, w_out, w_out2, m[r], v[r], step0, n, S)
    _launch(lib, dev, desc, T, W, second, S)
    return before, dict(theta=theta, saved=saved, m=m, v=v, shared=shared), alone


def _assert_six_equal(got, want, S, what):
    off = param_offsets(S)
    for a, name in enumerate(("W1", "b1", "W2", "b2", "W3", "b3")):
        sl = slice(int(off[a]), int(off[a + 1]))
        assert torch.equal(got[sl], want[sl]), f"{what}: {name} differs in {int((got[sl] != want[sl]).sum())} of {sl.stop - sl.start} elements"


@pytest.mark.parametrize("T,W", [(16, 1), (24, 2), (33, 1), (40, 1), (136, 1)])
@pytest.mark.parametrize("second", [1, 0], ids=["second_order", "first_order"])
@pytest.mark.parametrize("S", [64, 128])
def test_each_trial_is_bitwise_the_one_trial_call(lib, dev, S, second, T, W):
    """(16, 1): one partial chunk; (24, 2): a tail <= 16 with the word boundary inside a chunk; (33, 1): 32 + 1; (40, 1): a full
    32-row gradient chunk and a tail, 16 + 16 + 8 in the Hessian pass; (136, 1): nine 16-row Hessian chunks."""
    before, after, alone = _four_trials(lib, dev, S, T, W, second)
    for r in (0, 2, 3):
        th, m, v = alone[r]
        assert bool(torch.isfinite(th).all())
        _assert_six_equal(after["theta"][r], th, S, f"trial {r} weights")
        assert torch.equal(after["m"][r], m) and torch.equal(after["v"][r], v), f"trial {r} moments"
        assert not torch.equal(after["theta"][r], before["theta"][r]) and not torch.equal(after["m"][r], before["m"][r])
    assert torch.equal(after["saved"][0], before["saved"][0])  # w_out2 NULL: no second copy written anywhere near
    for r in (2, 3):
        _assert_six_equal(after["saved"][r], alone[r][0], S, f"trial {r} second copy")
    assert torch.equal(after["shared"], before["shared"])  # w_in is only read
    for name in ("theta", "saved", "m", "v"):  # the trial with n = 0 touched nothing
        assert bool((after[name][1] == SENTINEL).all()), name
    assert not torch.equal(after["theta"][0], after["theta"][2]) and not torch.equal(after["theta"][2], after["theta"][3])


def test_more_trials_than_cus(lib, dev):
    """R = CUs + 3 in one launch (gridDim.y = R): the trials beyond the first round start where one ends; four inputs cycled."""
    S, T, W = 128, 16, 1
    R = torch.cuda.get_device_properties(dev).multi_processor_count + 3
    w, rx, _, labels = _inputs(S, T)
    rxd, labd = torch.tensor(rx, device=dev), torch.tensor(labels.astype(np.int32), device=dev)
    base = torch.cat([torch.as_tensor(a).reshape(-1) for a in w]).to(dev)
    P = base.numel()
    gen = torch.Generator(device=dev).manual_seed(77)
    start = (base + 0.01 * torch.randn((4, P), generator=gen, device=dev)).contiguous()
    m0 = (1e-3 * torch.randn((4, P), generator=gen, device=dev)).contiguous()
    v0 = torch.empty((4, P), device=dev).uniform_(1e-7, 1e-5, generator=gen)
    steps = [_steps(1, W, 2 * k, dev) for k in range(4)]
    alone = [_alone(lib, dev, S, T, W, 1, rxd, labd, *steps[k], 1, start[k], m0[k], v0[k], 10 + k) for k in range(4)]
    which = torch.arange(R, device=dev) % 4
    theta, m, v = start[which].contiguous(), m0[which].contiguous(), v0[which].contiguous()
    desc = np.zeros(R, TRIAL_DTYPE)
    for r in range(R):
        _describe(desc[r:r + 1], rxd, labd, *steps[r % 4], theta[r], theta[r], None, m[r], v[r], 10 + r % 4, 1, S)
    _launch(lib, dev, desc, T, W, 1, S)
    for name, got, k in (("weights", theta, 0), ("exp_avg", m, 1), ("exp_avg_sq", v, 2)):
        want = torch.stack([a[k] for a in alone])[which]
        wrong = torch.nonzero((got != want).any(dim=1)).reshape(-1).tolist()
        assert not wrong, f"{name}: trials {wrong[:10]} of {R} differ from the one-trial call"
    assert len({bytes(a[0].cpu().numpy().tobytes()) for a in alone}) == 4  # four distinct results


@pytest.mark.parametrize("S", [64, 128])
def test_determinism(lib, dev, S):
    a = _four_trials(lib, dev, S, 40, 1, 1)[1]
    b = _four_trials(lib, dev, S, 40, 1, 1)[1]
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------- the engine
def _g21(golden, S, dev, blocks, R=3):
    """G21's flow at S states as R trials: the golden's words, then copies with fresh noise on rx (test_gpu_states_trials.py)."""
    g = golden("g21_by_word_meta_64_128_states")
    tag = f"L{STATES[S]}_meta"
    ss_it, meta_it, j_num, meta_sub, _, sub, nsym = [int(x) for x in g[f"{tag}_meta"]]
    assert ss_it == 6 and meta_sub == 5
    tx1 = torch.tensor(g[f"{tag}_tx"][:blocks], device=dev).float()
    rx1 = torch.tensor(g[f"{tag}_rx"][:blocks], device=dev)
    gen = torch.Generator(device=dev).manual_seed(64 + S)
    rx = torch.stack([rx1] + [rx1 + 0.15 * torch.randn(rx1.shape, generator=gen, device=dev) for _ in range(R - 1)]).contiguous()
    tx = tx1.unsqueeze(0).repeat(R, 1, 1).contiguous()
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    kw = dict(self_supervised=True, self_supervised_iterations=ss_it, ser_thresh=0.02, online_meta=True, meta_lr=META_LR,
              meta_train_iterations=meta_it, meta_j_num=j_num, meta_subframes=meta_sub, meta_style_online_training=True)
    return g, tag, w0, tx, rx, nsym, sub, kw


OWN = dict(MAML=True, window_size=1, weights_init="last_frame")  # G21's setting
OTHER = dict(MAML=False, window_size=2, weights_init="random", decision="path")


def _alone_run(S, w0, tx_r, rx_r, nsym, sub, draws, dev, kw):
    """harness.eval_by_word on one trial: (ser_by_word, weights, saved weights, exp_avg, exp_avg_sq, step, meta [N] bool)"""
    T = rx_r.shape[1]
    det = _vnet_with(w0, S, T, dev)
    tr = mvn.OnlineTrainer(det, STATES[S])
    last, meta = {}, np.zeros(rx_r.shape[0], bool)

    def observer(seen):
        if seen["stage"] == "end":
            meta[seen["count"]] = seen["meta"] is not None
            if seen["saved_detector"] is not None:
                last["saved"] = [p.detach().clone() for p in seen["saved_detector"].parameters()]

    ser = mvn.eval_by_word(det, tx_r, rx_r, 0.0, 0.0, nsym, sub, online_trainer=tr, draws=draws, observer=observer,
                           meta_detector=mvn.META_VNETDetector(S, {"train": T, "val": T}), **kw)
    w = [p.detach().clone() for p in det.parameters()]
    return ser, w, last.get("saved", w), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step, meta


def _assert_rows(bank, ser_b, rec, rows):
    for r, (ser, w, saved, m, v, step, meta) in enumerate(rows):
        assert np.array_equal(ser, ser_b[r]), (r, np.flatnonzero(ser != ser_b[r]))
        for a, b in zip(w, bank.weights(r)):
            assert torch.equal(a, b), f"trial {r}: weights"
        for a, b in zip(saved, bank.weights(r, saved=True)):
            assert torch.equal(a, b), f"trial {r}: saved weights"
        assert torch.equal(m, bank.exp_avg[r]) and torch.equal(v, bank.exp_avg_sq[r]), f"trial {r}: moments"
        assert step == int(bank.step[r]), (r, step, int(bank.step[r]))
        if rec is not None:
            assert np.array_equal(meta, rec["meta"][r]), (r, np.flatnonzero(meta), np.flatnonzero(rec["meta"][r]))


def _refuse_sequential(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the bank went trial after trial: the lock-step engine did not run")

    monkeypatch.setattr(trials, "_one_trial_at_a_time", refuse)


@pytest.mark.parametrize("setting", ["g21", "first_order_window2_random_path_cohorts2"])
@pytest.mark.parametrize("S", [64, 128])
def test_engine_rows_equal_sequential_runs(golden, dev, monkeypatch, S, setting):
    """R = 3 over the first 16 blocks of G21's flow (three updates of row 0): each row is harness.eval_by_word alone on that trial."""
    R = 3
    g, tag, w0, tx, rx, nsym, sub, kw = _g21(golden, S, dev, 16, R)
    kw.update(OWN if setting == "g21" else OTHER)
    rows = [_alone_run(S, w0, tx[r], rx[r], nsym, sub, TrialDraws(500 + r, dev), dev, kw) for r in range(R)]
    _refuse_sequential(monkeypatch)
    bank = TrialBank([w0] * R, S, STATES[S], dev)
    rec = {}
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, [TrialDraws(500 + r, dev) for r in range(R)], record=rec,
                                 cohorts=1 if setting == "g21" else 2, **kw)
    _assert_rows(bank, ser_b, rec, rows)
    print(f"S={S} {setting}: updates per row {rec['meta'].sum(axis=1).tolist()}, steps {bank.step.tolist()}")
    # updates ran (blocks 5, 10, 15 where the buffer held more than two words); the trials are not copies of each other
    assert rec["meta"][0].any() and not rec["meta"][:, :5].any() and len({tuple(row) for row in ser_b}) > 1
    assert np.array_equal(ser_b[0][:6], g[f"{tag}_ser_by_word"][:6]) or setting != "g21"  # row 0: the reference's run up to its first update


@pytest.mark.parametrize("S", [64, 128])
def test_g21_as_one_trial_among_three(golden, dev, monkeypatch, S):
    """All 50 blocks; row 0 has the reference's words and recorded draws: its ser_by_word is the reference's, its final and saved
    weights are within the bound of test_reference_meta_flow_64_128_states (the one-trial kernel's)."""
    R = 3
    g, tag, w0, tx, rx, nsym, sub, kw = _g21(golden, S, dev, 50, R)
    kw.update(OWN)
    _refuse_sequential(monkeypatch)
    bank = TrialBank([w0] * R, S, STATES[S], dev)
    draws = [RF._recorded(g, tag, dev)] + [TrialDraws(600 + r, dev) for r in range(1, R)]
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, draws, **kw)
    ref = g[f"{tag}_ser_by_word"]
    assert ser_b.shape == (R, 50)
    assert np.array_equal(ser_b[0], ref), (np.flatnonzero(ser_b[0] != ref), ser_b[0][ser_b[0] != ref], ref[ser_b[0] != ref])
    assert draws[0].used_up(), (draws[0].r_at, len(draws[0].randint))
    w = [a.cpu().numpy() for a in bank.weights(0)]
    saved = [a.cpu().numpy() for a in bank.weights(0, saved=True)]
    moved = max(float(np.abs(g[f"{tag}_w1_{i}"] - g[f"{tag}_w0_{i}"]).max()) for i in range(6))
    worst = max(float(np.abs(w[i] - g[f"{tag}_w1_{i}"]).max()) for i in range(6))
    worst_s = max(float(np.abs(saved[i] - g[f"{tag}_saved_{i}"]).max()) for i in range(6))
    print(f"g21 {tag} as row 0 of {R}: ser identical on 50 blocks; weights moved {moved:.4f}, end {worst:.2e} from the reference's, "
          f"saved weights {worst_s:.2e}")
    assert moved > 0.005 and worst <= G21_WEIGHT_TOL and worst_s <= G21_WEIGHT_TOL
    assert len({tuple(row) for row in ser_b}) > 1  # the trials are not copies of each other


def test_route(golden, dev, monkeypatch):
    """Default arguments: one trial goes through _one_trial_at_a_time (once), three take the engine.  meta_trial_axis=True puts the
    one trial on the engine, False sends the three trial after trial; the rows do not depend on the route."""
    S, R = 64, 3
    g, tag, w0, tx, rx, nsym, sub, kw = _g21(golden, S, dev, 16, R)
    kw.update(OWN)
    calls = []
    sequential = trials._one_trial_at_a_time

    def counted(*a, **k):
        calls.append(1)
        return sequential(*a, **k)

    monkeypatch.setattr(trials, "_one_trial_at_a_time", counted)

    def run(rows, **more):
        bank = TrialBank([w0] * len(rows), S, STATES[S], dev)
        rec = {}
        ser = eval_by_word_batched(bank, tx[rows], rx[rows], nsym, sub, [TrialDraws(500 + r, dev) for r in rows], record=rec, **kw, **more)
        return ser, bank, rec

    ser1, bank1, rec1 = run([1])
    assert calls == [1]
    ser1e, bank1e, rec1e = run([1], meta_trial_axis=True)
    assert calls == [1]  # the engine ran
    ser3, bank3, rec3 = run([0, 1, 2])
    assert calls == [1]
    ser3s, bank3s, rec3s = run([0, 1, 2], meta_trial_axis=False)
    assert calls == [1, 1]
    for (sa, ba, ra), (sb, bb, rb) in (((ser1, bank1, rec1), (ser1e, bank1e, rec1e)), ((ser3, bank3, rec3), (ser3s, bank3s, rec3s))):
        assert np.array_equal(sa, sb) and np.array_equal(ra["meta"], rb["meta"]) and np.array_equal(ba.step, bb.step)
        for name in ("theta", "saved", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(ba, name), getattr(bb, name)), name
    assert np.array_equal(ser1[0], ser3[1]) and torch.equal(bank1.theta[0], bank3.theta[1])
    assert rec1["meta"].any() and rec3["meta"][0].sum() == 3
