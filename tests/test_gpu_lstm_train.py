"""GPU: lstm_train_kernel (mvn_lstm_train_f32 behind LSTMOnlineTrainer) against torch autograd + torch.optim in float64 on the
CPU, against the autograd route on the same GPU and against golden G19; bit-reproducible across runs and across split calls;
the detector sees the trained weights; two trainers on two streams; the harness's update branch.  Tolerances and cases:
tests/test_lstm_train_host.py."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L
from test_lstm_host import g18_weights
from test_lstm_train_host import (CASE_NAMES, cases, check_case, check_g19_by_word, check_g19_part, check_losses,
                                  default_init_weights, detector_with, draw_batches, g19_by_word, g19_case, outside, referee, run_case,
                                  start_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lstm")


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _state(tr):
    return [p.detach().cpu().numpy() for p in tr.params] + [tr.exp_avg.cpu().numpy(), tr.exp_avg_sq.cpu().numpy()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_against_float64_referee(g18, name):
    c = cases(g18)[name]
    got, losses, tr, _ = run_case(c, DEV, use_kernel=True)
    assert tr.kernel_route(136) and tr.step == c["n"]
    assert int(tr.status.item()) == 0
    tr.check_status()
    check_case(name, c, got, losses)


@pytest.mark.parametrize("M", [8, 17])
def test_other_minibatch_sizes(g18, M):
    c = dict(cases(g18)["g18_minibatch_adam25"], idx=draw_batches(136, 25, M, 10 + M))
    got, losses, tr, _ = run_case(c, DEV, use_kernel=True)
    check_case(f"M{M}", c, got, losses)
    tr.check_status()


@pytest.mark.parametrize("T,full", [(40, False), (40, True), (256, True), (5, True)])
def test_other_word_lengths(T, full):
    rng = np.random.RandomState(T)
    bits = rng.randint(0, 2, (1, T))
    rx = ((1 - 2 * bits) + 0.4 * rng.randn(1, T)).astype(np.float32)
    n = 10
    c = dict(ws=default_init_weights(3), tx=bits, rx=rx, word_of_iter=None, idx=None if full else draw_batches(T, n, 16, T), n=n,
             optimizer_type="Adam", lr=1e-3)
    got, losses, tr, _ = run_case(c, DEV, use_kernel=True)
    assert tr.kernel_route(T)
    tr.check_status()
    ref, ref_losses, _ = referee(c["ws"], c["tx"], c["rx"], None, c["idx"], n)
    n_out, worst = outside(got, ref)
    print(f"T = {T}: {n_out} parameters outside the bound, largest deviation {worst:.3g}")
    assert n_out == 0
    check_losses(losses, ref_losses)


def test_word_longer_than_the_kernel_supports_takes_autograd():
    T = L.TRAIN_MAX_T + 8
    det = detector_with(default_init_weights(3), DEV)
    tr = mvn.LSTMOnlineTrainer(det, use_kernel=True)
    assert not tr.kernel_route(T)
    tr.online_training(torch.zeros(1, T, device=DEV), torch.randn(1, T, device=DEV), iterations=1, full_word=True)
    assert tr.step == 1


def test_state_carried_over_two_calls_against_referee(g18):
    c = cases(g18)["g18_minibatch_adam25"]
    det = detector_with(c["ws"], DEV)
    tr = mvn.LSTMOnlineTrainer(det, use_kernel=True)
    tx, rx = torch.from_numpy(c["tx"].astype(np.float32)).to(DEV), torch.from_numpy(c["rx"]).to(DEV)
    l1 = tr.online_training(tx, rx, iterations=10, batch_idx=c["idx"][:10], return_loss=True)
    l2 = tr.online_training(tx, rx, iterations=15, batch_idx=c["idx"][10:], return_loss=True)
    check_case("g18_minibatch_adam25", c, [p.detach().cpu().numpy() for p in tr.params], torch.cat([l1, l2]).cpu().numpy())
    tr.check_status()


@pytest.mark.parametrize("name", ["g18_minibatch_adam25", "g18_whole_word_adam12", "init_rmsprop8", "g18_joint_adam25"])
def test_bit_reproducible_and_split_calls(g18, name):
    c = cases(g18)[name]
    a, la, tra, _ = run_case(c, DEV, use_kernel=True)
    b, lb, trb, _ = run_case(c, DEV, use_kernel=True)
    assert _bits_equal(_state(tra), _state(trb)) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    # n1 + n2 in two calls
    n1 = c["n"] // 3
    det = detector_with(c["ws"], DEV)
    tr = mvn.LSTMOnlineTrainer(det, lr=c["lr"], optimizer_type=c["optimizer_type"], use_kernel=True)
    tx, rx = torch.from_numpy(c["tx"].astype(np.float32)).to(DEV), torch.from_numpy(c["rx"]).to(DEV)
    full = c["idx"] is None
    parts = []
    for lo, hi in ((0, n1), (n1, c["n"])):
        idx = None if full else c["idx"][lo:hi]
        if c["word_of_iter"] is None:
            parts.append(tr.online_training(tx, rx, iterations=hi - lo, batch_idx=idx, full_word=full, return_loss=True))
        else:
            parts.append(tr.train_words(tx[lo:hi], rx[lo:hi], batch_idx=idx, full_word=full, return_loss=True))
    assert _bits_equal(_state(tra), _state(tr))
    assert np.array_equal(torch.cat(parts).cpu().numpy().view(np.uint32), la.view(np.uint32))
    tr.check_status()


def test_more_iterations_than_one_launch_holds():
    """A call of more than 8192 iterations is issued as several launches with idx, word_of_iter, loss_out and the step number
    offset: bit-identical to the same iterations in calls that each fit one launch, minibatch and joint form."""
    T, n, cut = 5, 8192 + 9, 8192 - 3
    rng = np.random.RandomState(12)
    bits = torch.from_numpy(rng.randint(0, 2, (7, T)).astype(np.float32)).to(DEV)
    rx = ((1 - 2 * bits.cpu()) + 0.4 * torch.from_numpy(rng.randn(7, T).astype(np.float32))).to(DEV)
    idx = torch.from_numpy(rng.randint(0, T, (n, 3)).astype(np.int32))
    rows = torch.from_numpy(rng.randint(0, 7, n))
    ws = default_init_weights(3)
    for joint in (False, True):
        out = []
        for pieces in (((0, n),), ((0, cut), (cut, n))):
            det = detector_with(ws, DEV)
            tr = mvn.LSTMOnlineTrainer(det, use_kernel=True, lr=1e-4)  # (Adam: the bias corrections follow the step number)
            losses = []
            for lo, hi in pieces:
                if joint:
                    losses.append(tr.train_words(bits[rows[lo:hi]], rx[rows[lo:hi]], batch_idx=idx[lo:hi], return_loss=True))
                else:
                    losses.append(tr.online_training(bits[:1], rx[:1], iterations=hi - lo, batch_idx=idx[lo:hi], return_loss=True))
            tr.check_status()
            assert tr.step == n
            out.append((_state(tr), torch.cat(losses).cpu().numpy()))
        assert _bits_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
        assert np.isfinite(out[0][1]).all() and out[0][1][-1] != out[0][1][0]


@pytest.mark.parametrize("name", ["g18_minibatch_adam25", "g18_whole_word_adam12", "g18_sgd6", "init_rmsprop8", "g18_rmsprop3_minibatch"])
def test_kernel_and_autograd_routes_agree_on_the_gpu(g18, name):
    c = cases(g18)[name]
    a, la, _, _ = run_case(c, DEV, use_kernel=True)
    b, lb, trb, _ = run_case(c, DEV, use_kernel=False)
    assert not trb.kernel_route(136)
    n_out, worst = outside(a, [x.astype(np.float64) for x in b])
    print(f"{name}: kernel vs autograd route: {n_out} outside, largest deviation {worst:.3g}")
    assert n_out == 0
    check_losses(la, lb.astype(np.float64))


def test_detector_sees_the_trained_weights(g18):
    c = cases(g18)["g18_minibatch_adam25"]
    _, _, tr, det = run_case(c, DEV, use_kernel=True)
    rx = torch.from_numpy(g18["rx"][:20]).to(DEV)
    new = [p.detach().clone() for p in tr.params]
    assert not torch.equal(new[1].cpu(), torch.from_numpy(c["ws"][1]))
    dec, logits = L.lstm_decode(rx, new, return_logits=True)
    assert torch.equal(det(rx, "val"), dec)
    with torch.no_grad():
        got = det(rx, "train")
    lg = logits.cpu().numpy()
    assert np.all(np.abs(got.cpu().numpy() - lg) <= 1e-4 * (1 + np.abs(lg)))
    # and against a fresh module that never saw the kernel
    fresh = detector_with([w.cpu().numpy() for w in new], DEV)
    with torch.no_grad():
        assert torch.equal(fresh(rx, "train"), got)


def test_two_trainers_on_two_streams(g18):
    cs = cases(g18)
    ca, cb = cs["g18_minibatch_adam25"], cs["g18_whole_word_adam12"]
    alone_a, la, _, _ = run_case(ca, DEV, use_kernel=True)
    alone_b, lb, _, _ = run_case(cb, DEV, use_kernel=True)
    out = {}
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    torch.cuda.synchronize()
    for key, c, s in (("a", ca, streams[0]), ("b", cb, streams[1])):
        with torch.cuda.stream(s):
            out[key] = start_case(c, DEV, use_kernel=True)  # (nothing is read back before both are issued)
    torch.cuda.synchronize()
    for key, alone, l in (("a", alone_a, la), ("b", alone_b, lb)):
        tr, _, losses = out[key]
        got = [p.detach().cpu().numpy() for p in tr.params]
        assert _bits_equal(got, alone) and np.array_equal(losses.cpu().numpy().view(np.uint32), l.view(np.uint32))
        assert int(tr.status.item()) == 0
        tr.check_status()


@pytest.mark.parametrize("part", ["a", "b"])
def test_g19_online_training_through_the_kernel(golden, g18, part):
    g19 = golden("g19_lstm_train")
    got, losses, tr, _ = run_case(g19_case(g19, g18, part), DEV, use_kernel=True)
    tr.check_status()
    check_g19_part(g19, part, got, losses)


@pytest.mark.parametrize("use_kernel", [True, False])
def test_g19_by_word_update_branch(golden, g18, use_kernel):
    g19 = golden("g19_lstm_train")
    det = detector_with(g18_weights(g18), DEV)
    tr = mvn.LSTMOnlineTrainer(det, use_kernel=use_kernel)
    ser, trained = g19_by_word(g19, g18, det, tr, DEV)
    check_g19_by_word(g19, ser, trained)
    assert tr.step == 8 * len(trained) and int(tr.status.item()) == 0


def test_meta_style_update_branch_restores_saved_weights(golden, g18):
    g19 = golden("g19_lstm_train")
    ws = g18_weights(g18)
    det = detector_with(ws, DEV)
    tr = mvn.LSTMOnlineTrainer(det, use_kernel=True)
    tx, rx = torch.from_numpy(g19["c_tx"][:4].astype(np.float32)).to(DEV), torch.from_numpy(g19["c_rx"][:4]).to(DEV)
    seen = []
    mvn.eval_by_word(det, tx, rx, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, self_supervised=True, online_trainer=tr,
                     self_supervised_iterations=2, ser_thresh=1.0, meta_style_online_training=True, observer=seen.append)
    ends = [s for s in seen if s["stage"] == "end"]
    assert [s["trained"] for s in ends] == [True] * 4 and tr.step == 8
    det2 = detector_with(ws, DEV)
    tr2 = mvn.LSTMOnlineTrainer(det2, use_kernel=True)
    for s in ends:  # every block's training starts from the weights the run started with; the optimizer state runs through
        with torch.no_grad():
            for p, w in zip(tr2.params, ws):
                p.copy_(torch.from_numpy(w))
        tr2.online_training(s["buffer_tx"][-1].reshape(1, -1), s["buffer_rx"][-1].reshape(1, -1), iterations=2, full_word=True)
    assert all(torch.equal(a, b) for a, b in zip(tr.params, tr2.params))


def test_harness_refusals_on_the_gpu(g18):
    det = detector_with(g18_weights(g18), DEV)
    tx, rx = torch.zeros(3, 120, device=DEV), torch.zeros(3, 136, device=DEV)
    with pytest.raises(ValueError, match="LSTMOnlineTrainer"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, self_supervised=True)
    with pytest.raises(ValueError, match="LSTM"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, online_meta=True,
                         online_trainer=mvn.LSTMOnlineTrainer(det))
