"""The word axis of the one-launch ViterbiNet training kernel (online_train_words_kernel, mvn_vnet_train_words_f32) on the device:
against the autograd route at the shapes where its two-stage prefetch can go wrong, bit for bit against the one-word kernel it
shares its body with, and the reference's joint-training and meta-training flows (G22) through mvn.joint_train / mvn.meta_train
on the kernel route.  Tolerance: the project's training tolerance (tests/test_gpu_parity.py), loss rtol 2e-4 / atol 1e-6 and
|dw| <= 2e-5 + 1e-3 |w|."""
import copy

import pytest
import torch

import meta_viterbinet_amd as mvn
import train_words_cases as cases

pytestmark = pytest.mark.gpu

STATES = (4, 16, 32, 64, 128)
WORD_OF_ITER = (3, 0, 3, 4, 1)  # not monotone, word 3 twice, word 2 never
# (T, K, M); M = 0: the whole word.  K < T with the reference's minibatch; one sample; 33 and 40 samples = a second, short chunk
# (1 and 8 rows: the 16-row form); whole words of 33 symbols (a chunk of one sample) and of 64 (two full chunks)
SHAPES = [(136, 120, 32), (136, 120, 1), (136, 120, 33), (136, 120, 40), (33, 33, 0), (64, 64, 0)]
OPTIMIZERS = {"Adam": 5e-3, "RMSprop": 2e-3, "SGD": 0.1}
CASES = [(S, kind) for S in STATES for kind in OPTIMIZERS if kind == "Adam" or S in (16, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _setup(dev, S, T, K, M, kind, n_words=5, n_iter=5, seed=0):
    """Two detectors with the same weights (kernel route, autograd route), words and draws."""
    L = S.bit_length() - 1
    gen = torch.Generator().manual_seed(1000 * S + 10 * T + M + seed)
    tx = torch.randint(0, 2, (n_words, K), generator=gen).float().to(dev)
    rx = torch.randn(n_words, T, generator=gen).to(dev)
    idx = torch.stack([torch.randperm(K, generator=gen)[:M] for _ in range(n_iter)]).to(dev) if M else None
    torch.manual_seed(S + seed)
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    twin = copy.deepcopy(det)
    lr = OPTIMIZERS[kind]
    return (tx, rx, idx, det, mvn.OnlineTrainer(det, L, lr=lr, optimizer_type=kind),
            twin, mvn.OnlineTrainer(twin, L, lr=lr, optimizer_type=kind, use_kernel=False))


def _state_close(tr, ref, what):
    for k, (p, q) in enumerate(zip(tr.params, ref.params)):
        cases.weights_close(p.detach().cpu().numpy(), q.detach().cpu().numpy(), f"{what} tensor {k}")
    cases.weights_close(tr.exp_avg.cpu().numpy(), ref.exp_avg.cpu().numpy(), f"{what} exp_avg")
    cases.weights_close(tr.exp_avg_sq.cpu().numpy(), ref.exp_avg_sq.cpu().numpy(), f"{what} exp_avg_sq")
    assert tr.step == ref.step


def _state_equal(tr, ref):
    for p, q in zip(tr.params, ref.params):
        assert torch.equal(p, q)
    assert torch.equal(tr.exp_avg, ref.exp_avg) and torch.equal(tr.exp_avg_sq, ref.exp_avg_sq) and tr.step == ref.step


@pytest.mark.parametrize("T,K,M", SHAPES)
@pytest.mark.parametrize("S,kind", CASES)
def test_word_axis_against_autograd(dev, S, kind, T, K, M):
    """Five steps on words 3, 0, 3, 4, 1 of five: the word of the chunk being prefetched is not the word of the chunk being computed."""
    tx, rx, idx, det, tr, twin, ref = _setup(dev, S, T, K, M, kind)
    assert tr.words_kernel_route() and not ref.words_kernel_route()
    woi = torch.tensor(WORD_OF_ITER, dtype=torch.int32)
    got = tr._train_words(tx, rx, woi, idx, M == 0, True)
    want = ref._train_words(tx, rx, woi, idx, M == 0, True)
    torch.cuda.synchronize()
    cases.losses_close(got.cpu().numpy(), want.cpu().numpy(), f"S={S} {kind} T={T} K={K} M={M} losses")
    _state_close(tr, ref, f"S={S} {kind} T={T} K={K} M={M}")
    assert bool(torch.isfinite(got).all()) and bool((got > 0).all())


@pytest.mark.parametrize("S", STATES)
def test_one_word_in_one_step(dev, S):
    """n = 1: both prefetches that run ahead of the first chunk already look past the last iteration."""
    for T, K, M in ((136, 120, 32), (33, 33, 0)):
        tx, rx, idx, det, tr, twin, ref = _setup(dev, S, T, K, M, "Adam", n_words=1, n_iter=1)
        got = tr.train_words(tx, rx, batch_idx=idx, full_word=M == 0, return_loss=True)
        want = ref.train_words(tx, rx, batch_idx=idx, full_word=M == 0, return_loss=True)
        cases.losses_close(got.cpu().numpy(), want.cpu().numpy(), f"S={S} n=1 M={M} loss")
        _state_close(tr, ref, f"S={S} n=1 M={M}")


@pytest.mark.parametrize("M", [32, 0], ids=["minibatch", "whole_word"])
@pytest.mark.parametrize("S,kind", CASES)
def test_identical_rows_equal_online_training(dev, S, kind, M):
    """Five identical rows, step i on row i, against online_training(iterations=5) on that row with the same draws: the same
    weights, moments and losses bit for bit (the two kernels share their body; the one-word call may spread a whole word over
    workgroups, which is bit-identical to the single workgroup by that form's own contract)."""
    T = 136
    tx, rx, idx, det, tr, twin, _ = _setup(dev, S, T, T, M, kind, n_words=1)
    one = mvn.OnlineTrainer(twin, tr.memory_length, lr=tr.lr, optimizer_type=kind)
    got = tr.train_words(tx.repeat(5, 1), rx.repeat(5, 1), batch_idx=idx, full_word=M == 0, return_loss=True)
    want = one.online_training(tx, rx, iterations=5, batch_idx=idx, full_word=M == 0, return_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    _state_equal(tr, one)
    assert bool((got > 0).all()) and tr.step == 5


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("kind", ["SGD", "RMSprop", "Adam"])
def test_five_words_equal_five_chained_calls(dev, S, kind):
    """train_words on five different words against five one-iteration online_training calls with the state carried over.  SGD and
    RMSprop have no running bias power: bit for bit.  With Adam the host hands every call pow(beta, step0) while the kernel
    multiplies its running product by beta once per iteration -- the two doubles need not agree to the last bit, so Adam is held to
    the tolerance only."""
    T, M = 136, 32
    tx, rx, idx, det, tr, twin, _ = _setup(dev, S, T, T, M, kind)
    one = mvn.OnlineTrainer(twin, tr.memory_length, lr=tr.lr, optimizer_type=kind)
    got = tr.train_words(tx, rx, batch_idx=idx, return_loss=True)
    want = torch.cat([one.online_training(tx[i:i + 1], rx[i:i + 1], iterations=1, batch_idx=idx[i:i + 1], return_loss=True)
                      for i in range(5)])
    torch.cuda.synchronize()
    if kind == "Adam":
        cases.losses_close(got.cpu().numpy(), want.cpu().numpy(), f"S={S} Adam chained losses")
        _state_close(tr, one, f"S={S} Adam chained")
    else:
        assert torch.equal(got, want)
        _state_equal(tr, one)


def test_no_iterations_touch_nothing(dev):
    """n_iter == 0 returns MVN_OK before anything is launched: loss_out keeps its sentinel, weights and moments their values."""
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    tx, rx, idx, det, tr, twin, _ = _setup(dev, 16, 136, 120, 32, "Adam")
    labels = mvn.calculate_states(4, tx).reshape(5, 120).to(torch.int32).contiguous()
    woi = torch.arange(5, dtype=torch.int32, device=dev)
    loss = torch.full((5,), -7.5, device=dev)
    tr.exp_avg.fill_(0.25)
    tr.exp_avg_sq.fill_(0.5)
    with torch.cuda.device(dev):
        rc = lib.mvn_vnet_train_words_f32(ptr(rx), 136, ptr(labels), 120, 5, 120, ptr(woi), ptr(idx.to(torch.int32).contiguous()), 32, 0,
                                          *[ptr(t.data) for t in tr.params], ptr(tr.exp_avg), ptr(tr.exp_avg_sq), 0, 1e-3, 0.9, 0.999,
                                          1e-8, ptr(loss), 16, mvn._lib.current_stream(dev))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((loss == -7.5).all())
    for p, q in zip(det.parameters(), twin.parameters()):
        assert torch.equal(p, q)
    assert bool((tr.exp_avg == 0.25).all()) and bool((tr.exp_avg_sq == 0.5).all())


@pytest.mark.parametrize("tag", sorted(cases.JOINT_FLOWS))
def test_joint_train_replays_g22_on_the_kernel(dev, tag):
    """VNETTrainer.train() as the reference ran it, every minibatch's 25 steps in one launch, the validations on the device (detect,
    RS decode, count): the same error counts and best minibatch, per-step and per-minibatch losses and the weights within tolerance."""
    cases.replay_joint(tag, dev, use_kernel=True)


@pytest.mark.parametrize("tag", sorted(cases.META_FLOWS))
def test_meta_train_replays_g22_on_the_kernel(dev, tag):
    """METAVNETTrainer.meta_train() as the reference ran it, every minibatch's steps in one launch of the meta-learning kernel."""
    cases.replay_meta(tag, dev, use_kernel=True)
