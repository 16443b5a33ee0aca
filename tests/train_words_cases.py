"""What tests/test_train_words_host.py (autograd route, CPU) and tests/test_gpu_train_words.py (kernel route) share: the G22 fixture
(tests/golden/g22_joint_training.npz, written by tests/golden/make_golden_joint_train.py from the unmodified reference), the replay
of its flows through mvn.joint_train / mvn.meta_train, and the project's training tolerance (tests/test_gpu_parity.py: loss rtol 2e-4 /
atol 1e-6, |dw| <= 2e-5 + 1e-3 |w|)."""
import os

import numpy as np
import torch

import meta_viterbinet_amd as mvn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_joint_training.npz")
LOSS_RTOL, LOSS_ATOL = 2e-4, 1e-6
W_ATOL, W_RTOL = 2e-5, 1e-3
W2_POS = np.random.RandomState(2200).choice(5000, 512, replace=False)  # the digest's sample of W2 (make_golden_joint_train.py)
JOINT_FLOWS = {"a_adam": "Adam", "a_rmsprop": "RMSprop", "a_sgd": "SGD"}
META_FLOWS = {"b_maml": True, "b_fo": False}

_g22 = None


def g22():
    global _g22
    if _g22 is None:
        with np.load(GOLDEN) as z:
            _g22 = {k: z[k] for k in z.files}
    return _g22


def weights_close(got, want, what=""):
    """|got - want| <= 2e-5 + 1e-3 |want| element by element; prints the largest excess ratio first."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = float((np.abs(got - want) / (W_ATOL + W_RTOL * np.abs(want))).max()) if got.size else 0.0
    print(f"{what}: largest |dw| / (2e-5 + 1e-3 |w|) = {ratio:.4g}, largest |dw| = {float(np.abs(got - want).max()):.3g}")
    assert ratio <= 1.0, f"{what}: weights off by {ratio:.3g} x the tolerance"


def losses_close(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print(f"{what}: largest |dloss| = {float(err.max()):.3g} (largest relative {float((err / np.abs(want)).max()):.3g})")
    np.testing.assert_allclose(got, want, rtol=LOSS_RTOL, atol=LOSS_ATOL, err_msg=what)


def ser_close(got, want):
    """The reference's ser is 1 - (a float32 mean of the matches) (metrics.py:13-16): within 2^-23 of errors / bits, which is what the
    counters give; the integers themselves are compared exactly."""
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=0, atol=2.0 ** -23)


def digest_close(weights, g, prefix):
    """A list of six weight tensors against the fixture's digest `prefix` (five tensors whole, 512 entries of W2 and its norm)."""
    for k, w in enumerate(weights):
        w = w.detach().cpu().numpy().astype(np.float64).reshape(-1)
        if k == 2:
            weights_close(w[W2_POS], g[f"{prefix}_p2"], f"{prefix} W2 sample")
            norm, want = float(np.linalg.norm(w)), float(g[f"{prefix}_n2"])
            assert abs(norm - want) <= W_ATOL * np.sqrt(w.size) + W_RTOL * want, (prefix, norm, want)
        else:
            weights_close(w, g[f"{prefix}_p{k}"], f"{prefix} tensor {k}")


def fresh_detector(dev, optimizer_type, lr, use_kernel=True):
    """A 16-state detector holding the fixture's initial weights, and its trainer (memory 4, minibatches of 32)."""
    g = g22()
    det = mvn.VNETDetector(16, {"train": 136, "val": 136}).to(dev)
    with torch.no_grad():
        for p, k in zip(det.parameters(), range(6)):
            p.copy_(torch.from_numpy(g[f"w0_{k}"]))
    return det, mvn.OnlineTrainer(det, 4, lr=lr, optimizer_type=optimizer_type, use_kernel=use_kernel)


def recorded_words(dev):
    """words(minibatch, phase) replaying the fixture's words on `dev`"""
    g = g22()

    def words(mb, phase):
        return (torch.from_numpy(g[f"{phase}_tx"][mb].astype(np.float32)).to(dev), torch.from_numpy(g[f"{phase}_rx"][mb]).to(dev))

    return words


def oracle_evaluate(detector, tx, rx):
    """single_eval_at_point for a CPU detector: the CPU oracle's ViterbiNet decode and RS decode, errors over the data rows."""
    import oracle

    w = [p.detach().cpu().numpy() for p in detector.parameters()]
    msg = oracle.rs_decode_bits(oracle.vnet_decode(rx.cpu().numpy(), w), 2)
    rows = np.array([i for i in range(tx.shape[0]) if i % 25 != 0], np.int64)
    counters = oracle.count_errors(msg, tx.cpu().numpy(), rows)
    return oracle.error_rates(counters)[0], counters


def oracle_encode(tx, n_symbols):
    import oracle

    return torch.from_numpy(oracle.rs_encode_bits(tx.cpu().numpy(), n_symbols))


def replay_joint(tag, dev, use_kernel, evaluate=None):
    """Part a of G22 through mvn.joint_train with the recorded words and draws; asserts what both routes must show."""
    g = g22()
    det, tr = fresh_detector(dev, JOINT_FLOWS[tag], float(g[f"{tag}_lr"]), use_kernel)
    res = mvn.joint_train(det, tr, 10.0, 0.2, 3, words=recorded_words(dev), n_symbols=2, subframes_in_frame=25,
                          batch_idx=g[f"{tag}_idx"].astype(np.int64), evaluate=evaluate)
    print(tag, "errors", res.counters[:, 0].tolist(), "recorded", g[f"{tag}_errors"].tolist(), "best", res.best_minibatch)
    assert res.counters[:, 0].tolist() == g[f"{tag}_errors"].tolist()  # exact: the fixture's condition
    assert res.best_minibatch == int(g[f"{tag}_best"])
    ser_close(res.ser, g[f"{tag}_ser"])
    assert res.best_ser == res.ser[res.best_minibatch]
    assert tr.step == 75
    losses_close(res.step_losses, g[f"{tag}_loss"], f"{tag} step losses")
    losses_close(res.losses, g[f"{tag}_loss"].sum(axis=1), f"{tag} minibatch losses")
    digest_close(list(det.parameters()), g, f"{tag}_final")
    digest_close(res.best_weights, g, f"{tag}_best" if int(g[f"{tag}_best"]) != 2 else f"{tag}_final")
    return res


def replay_meta(tag, dev, use_kernel, evaluate=None, encode=None):
    """Part b of G22 through mvn.meta_train with the recorded words and j_hat values."""
    g = g22()
    det, tr = fresh_detector(dev, "Adam", float(g[f"{tag}_lr"]), use_kernel)
    meta_det = mvn.META_VNETDetector(16, {"train": 136, "val": 136})
    j_hat = [np.unique(r) for r in g[f"{tag}_randint"]]  # torch.unique sorts, like numpy's
    res = mvn.meta_train(det, meta_det, tr, 10.0, 0.2, 3, words=recorded_words(dev), n_symbols=2, subframes_in_frame=25,
                         window_size=1, meta_j_num=4, meta_lr=float(g[f"{tag}_meta_lr"]), MAML=META_FLOWS[tag], j_hat=j_hat,
                         evaluate=evaluate, encode=encode)
    print(tag, "errors", res.counters[:, 0].tolist(), "recorded", g[f"{tag}_errors"].tolist())
    assert res.counters[:, 0].tolist() == g[f"{tag}_errors"].tolist()  # exact: the fixture's condition
    ser_close(res.ser, g[f"{tag}_ser"])
    assert tr.step == sum(len(j) for j in j_hat)
    for mb in range(3):
        want = g[f"{tag}_loss"][mb]
        want = want[~np.isnan(want)]
        assert len(want) == len(j_hat[mb]) and res.j_hat[mb].tolist() == j_hat[mb].tolist()
        losses_close(res.step_losses[mb], want, f"{tag} query losses of minibatch {mb}")
        assert abs(res.losses[mb] - want.sum()) <= LOSS_RTOL * want.sum() + LOSS_ATOL
    assert len(res.weights) == 3  # saved after every minibatch
    digest_close(res.weights[2], g, f"{tag}_final")
    digest_close(list(det.parameters()), g, f"{tag}_final")
    return res
