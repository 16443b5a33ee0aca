"""CPU only: joint training and offline meta-training of ViterbiNet as far as they can be seen without a device -- the argument
validation of mvn_vnet_train_words_f32 (no case reaches a launch), OnlineTrainer.train_words on the autograd route against a loop
over torch.optim written out by hand, and mvn.joint_train / mvn.meta_train on that route replaying the reference's recorded flows
(G22, tests/golden/g22_joint_training.npz; the detection of the validations runs on the CPU oracle)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import meta_viterbinet_amd as mvn
import train_words_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_STATES, E_NULL = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch


def _call(lib, y=P, y_ld=136, labels=P, lab_ld=120, n_words=5, K=120, woi=P, idx=P, M=32, n_iter=5, w=(P,) * 6, m=P, v=P, step0=0,
          S=16, beta1=0.9):
    return lib.mvn_vnet_train_words_f32(y, y_ld, labels, lab_ld, n_words, K, woi, idx, M, n_iter, *w, m, v, step0, 1e-3, beta1, 0.999,
                                        1e-8, None, S, None)


def test_error_ladder(lib):
    """MVN_E_DIMS, then MVN_E_STATES, then MVN_OK for n_iter == 0, then MVN_E_NULL -- each rung with everything below it wrong too."""
    null = dict(y=None, labels=None, woi=None, w=(None,) * 6, m=None, v=None)
    for bad in (dict(n_iter=-1), dict(n_words=0), dict(K=0), dict(K=137), dict(K=121), dict(M=-1), dict(M=121), dict(y_ld=119),
                dict(lab_ld=119), dict(step0=-1)):
        assert _call(lib, **bad) == E_DIMS, bad
        assert _call(lib, **dict(bad, S=256, **null)) == E_DIMS, bad  # shapes before states before pointers
        if "n_iter" not in bad:
            assert _call(lib, **dict(bad, n_iter=0)) == E_DIMS, bad
    for S in (0, 1, 3, 24, 256, 512):
        assert _call(lib, S=S) == E_STATES, S
        assert _call(lib, S=S, n_iter=0, **null) == E_STATES, S
    for S in (2, 4, 8, 16, 32, 64, 128):
        assert _call(lib, S=S, n_iter=0, **null) == OK, S  # nothing to do: nothing is looked at
    for missing in ("y", "labels", "woi", "m", "v"):
        assert _call(lib, **{missing: None}) == E_NULL, missing
    for a in range(6):
        assert _call(lib, w=tuple(None if k == a else P for k in range(6))) == E_NULL, a
    for beta1 in (0.9, -1.0, -2.0):  # Adam and the RMSprop / SGD tags all pass the checks
        assert _call(lib, beta1=beta1, y=None) == E_NULL
    # the edges that are allowed: K = both strides, M = K, M = 0 with or without a batch_idx
    assert _call(lib, K=120, y_ld=120, M=120, y=None) == E_NULL
    assert _call(lib, M=0, idx=None, y=None) == E_NULL and _call(lib, M=0, y=None) == E_NULL


def test_binding_and_header_agree(lib):
    """The symbol is declared once, exported, and bound with one ctypes type per parameter of the declaration."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvn.h")).read(), flags=re.S)
    decl = re.findall(r"int\s+mvn_vnet_train_words_f32\s*\(([^)]*)\)", text)
    assert len(decl) == 1
    params = [p.strip() for p in decl[0].split(",")]
    res, args = mvn._lib.SIGNATURES["mvn_vnet_train_words_f32"]
    assert res is ctypes.c_int and len(args) == len(params) == 26
    for p, a in zip(params, args):
        want = (ctypes.c_void_p if "*" in p or p.startswith("mvn_stream_t") else ctypes.c_int64 if p.startswith("int64_t") else
                ctypes.c_int32 if p.startswith("int32_t") else ctypes.c_float if p.startswith("float") else None)
        assert a is want, (p, a)
    assert hasattr(ctypes.CDLL(mvn._lib.LIB_PATH), "mvn_vnet_train_words_f32")
    assert lib.mvn_version() == 6  # an added entry point, no ABI bump
    assert callable(mvn.joint_train) and callable(mvn.meta_train) and callable(mvn.OnlineTrainer.train_words)


def _torch_optimizer(kind, params, lr):
    if kind == "Adam":
        return torch.optim.Adam(params, lr=lr)
    if kind == "RMSprop":
        return torch.optim.RMSprop(params, lr=lr)
    return torch.optim.SGD(params, lr=lr)


# n = 5 words; (T, K, M): K < T with the reference's minibatch, one sample per step, the whole word
SHAPES = [(136, 120, 32), (136, 120, 1), (40, 40, 0), (33, 20, 7)]


@pytest.mark.parametrize("kind,lr", [("Adam", 5e-3), ("RMSprop", 2e-3), ("SGD", 0.1)])
@pytest.mark.parametrize("T,K,M", SHAPES)
def test_train_words_equals_a_torch_optim_loop(kind, lr, T, K, M):
    """train_words on a CPU detector against `for each word: CE over the drawn positions of the first K logits; backward; step` on
    torch.optim.  The two compute the same operations in the same order; the trainer's own update (optimizer_step) and torch's may
    round an operation differently (fused / foreach forms), so: per step and element at most ~6 roundings of 2^-24 relative on an
    update of size <= lr x O(1), and one of 2^-24 on the weight itself -- over n = 5 steps |dw| <= 5 (2^-23 |w| + 6 x 2^-24 lr x 4)."""
    n, S, L = 5, 16, 4
    gen = torch.Generator().manual_seed(100 * T + M)
    tx = torch.randint(0, 2, (n, K), generator=gen).float()
    rx = torch.randn(n, T, generator=gen)
    idx = torch.stack([torch.randperm(K, generator=gen)[:M] for _ in range(n)]) if M else None
    torch.manual_seed(7)
    det = mvn.VNETDetector(S, {"train": T, "val": T})
    twin = mvn.VNETDetector(S, {"train": T, "val": T})
    twin.load_state_dict(det.state_dict())
    start = [p.detach().clone() for p in det.parameters()]
    tr = mvn.OnlineTrainer(det, L, lr=lr, optimizer_type=kind)
    assert not tr.words_kernel_route()
    got = tr.train_words(tx, rx, batch_idx=idx, full_word=M == 0, return_loss=True)
    assert tr.step == n and got.shape == (n,)

    opt = _torch_optimizer(kind, twin.parameters(), lr)
    labels = mvn.calculate_states(L, tx).reshape(n, K)
    want = []
    for i in range(n):
        logits = twin(rx[i:i + 1], "train").reshape(-1, S)[:K]
        loss = F.cross_entropy(logits, labels[i]) if M == 0 else F.cross_entropy(logits[idx[i]], labels[i][idx[i]])
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(loss.detach())
    np.testing.assert_allclose(got.numpy(), torch.stack(want).numpy(), rtol=cases.LOSS_RTOL, atol=cases.LOSS_ATOL)
    moved = 0.0
    for p, q, p0 in zip(det.parameters(), twin.parameters(), start):
        a, b = p.detach().double(), q.detach().double()
        bound = n * (2.0 ** -23 * b.abs() + 6 * 2.0 ** -24 * lr * 4)
        assert bool(((a - b).abs() <= bound).all()), float(((a - b).abs() / bound).max())
        moved = max(moved, float((a - p0.detach().double()).abs().max()))
    assert moved > 10 * lr * 2.0 ** -10  # (the steps did something)


def test_train_words_checks_its_shapes():
    det = mvn.VNETDetector(16, {"train": 40, "val": 40})
    tr = mvn.OnlineTrainer(det, 4)
    tx, rx = torch.zeros(3, 40), torch.zeros(3, 40)
    with pytest.raises(ValueError):
        tr.train_words(torch.zeros(3, 41), rx)  # K > T
    with pytest.raises(ValueError):
        tr.train_words(torch.zeros(3, 32), rx, full_word=True)  # the whole word needs K == T
    with pytest.raises(ValueError):
        tr.train_words(torch.zeros(2, 40), rx)  # a word per row in both
    with pytest.raises(ValueError):
        tr.train_words(tx, rx, batch_idx=torch.zeros(2, 8, dtype=torch.int64))  # a row of draws per word
    assert tr.step == 0
    assert tr.train_words(tx[:0], rx[:0], full_word=True, return_loss=True).shape == (0,) and tr.step == 0  # no words: no steps


@pytest.mark.parametrize("tag", sorted(cases.JOINT_FLOWS))
def test_joint_train_replays_g22_on_autograd(tag):
    """VNETTrainer.train() as the reference ran it (3 minibatches x 25 words, K = 120 of T = 136, recorded words and draws): the same
    error counts and best minibatch, losses and weights within the training tolerance."""
    res = cases.replay_joint(tag, "cpu", use_kernel=False, evaluate=cases.oracle_evaluate)
    assert res.step_losses.shape == (3, 25)


@pytest.mark.parametrize("tag", sorted(cases.META_FLOWS))
def test_meta_train_replays_g22_on_autograd(tag):
    """METAVNETTrainer.meta_train() as the reference ran it (second and first order), through meta.meta_train_loop."""
    cases.replay_meta(tag, "cpu", use_kernel=False, evaluate=cases.oracle_evaluate, encode=cases.oracle_encode)


def test_best_weights_rule_is_strict():
    """ser < best_ser: a later minibatch with the SAME ser does not replace the kept weights; the first always wins against inf."""
    det = mvn.VNETDetector(16, {"train": 16, "val": 16})
    tr = mvn.OnlineTrainer(det, 4, lr=0.05, optimizer_type="SGD")
    gen = torch.Generator().manual_seed(3)

    def words(mb, phase):
        return torch.randint(0, 2, (2, 16), generator=gen).float(), torch.randn(2, 16, generator=gen)

    sers = iter([0.25, 0.25, 0.125, 0.125, 0.5])
    seen = []

    def evaluate(detector, tx, rx):
        seen.append([p.detach().clone() for p in detector.parameters()])
        return next(sers), np.zeros(4, np.int64)

    res = mvn.joint_train(det, tr, 10.0, 0.2, 5, words=words, full_word=True, evaluate=evaluate)
    assert res.ser.tolist() == [0.25, 0.25, 0.125, 0.125, 0.5]
    assert res.best_minibatch == 2 and res.best_ser == 0.125
    assert all(torch.equal(a, b) for a, b in zip(res.best_weights, seen[2]))
    assert not all(torch.equal(a, b) for a, b in zip(res.best_weights, seen[3]))  # (the weights did move on)
    assert not all(torch.equal(a, b) for a, b in zip(res.best_weights, det.parameters()))
    one = mvn.joint_train(det, tr, 10.0, 0.2, 1, words=words, full_word=True, evaluate=lambda d, t, r: (1.0, np.zeros(4, np.int64)))
    assert one.best_minibatch == 0 and one.best_ser == 1.0  # the first minibatch wins against inf, whatever its ser
