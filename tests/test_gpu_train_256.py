"""GPU: several optimizer steps of online_train_kernel<256, false> (channel memory 8, 256 trellis states; trainer.py:163-185 takes
any memory_length) against torch autograd + torch.optim on the same word and draws, in the style of
tests/test_gpu_parity.py::test_online_training_at_64_and_128_states_vs_torch and with its tolerances: Adam, RMSprop and SGD,
minibatches of 17, 32 and 70 positions and the whole word, the optimizer state carried over two calls.  At this state count W3's
gradient reaches the optimizer from registers and W3's moments are updated in the accumulators' element order
(csrc/online_train.inc: apply_dw3_from_regs), every other element as at 64 / 128 states.
tests/test_gpu_vnet_grad_256.py holds the gradient itself, element by element."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from test_gpu_parity import _np, _rand_weights, _torch_online_ref, _vnet_with

pytestmark = pytest.mark.gpu
S, L, T = 256, 8, 136


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("n_iter,full_word,M,optimizer", [(1, False, 32, "Adam"), (8, False, 32, "Adam"), (3, True, 32, "Adam"), (5, False, 17, "Adam"),
                                                         (4, False, 70, "Adam"), (6, False, 32, "RMSprop"), (3, True, 32, "SGD")])
def test_online_training_at_256_states_vs_torch(dev, n_iter, full_word, M, optimizer):
    rng = np.random.RandomState(S + n_iter + M)
    w = _rand_weights(S, rng)
    tx = rng.randint(0, 2, (1, T)).astype(np.float32)
    y = rng.normal(0, 1.5, (1, T)).astype(np.float32)
    labels = mvn.calculate_states(L, torch.tensor(tx)).numpy()
    assert labels.max() >= S // 2  # the labels use the upper half of the states
    idx = np.stack([rng.choice(np.arange(1, T), M, replace=False) for _ in range(n_iter)]).astype(np.int32)
    lr = 0.05 if optimizer == "SGD" else 1e-3
    ref_w, ref_loss = _torch_online_ref(w, y[0], labels, idx, lr, n_iter, full_word, optimizer)
    det = _vnet_with(w, S, T, dev)
    tr = mvn.OnlineTrainer(det, L, lr=lr, optimizer_type=optimizer)
    name = ctypes.create_string_buffer(96)
    assert mvn._lib.load().mvn_vnet_train_kernel_name(0, 0, T, 0 if full_word else M, S, 1 << 22, name, 96) == 0
    assert name.value.decode() == "online_train_kernel<256, false> 1x1"
    n1 = n_iter // 2
    l1 = tr.online_training(torch.tensor(tx, device=dev), torch.tensor(y, device=dev), iterations=n1,
                            batch_idx=torch.tensor(idx[:n1], device=dev), full_word=full_word, return_loss=True) if n1 else None
    l2 = tr.online_training(torch.tensor(tx, device=dev), torch.tensor(y, device=dev), iterations=n_iter - n1,
                            batch_idx=torch.tensor(idx[n1:], device=dev), full_word=full_word, return_loss=True)
    assert tr.step == n_iter
    loss = np.concatenate([_np(l1), _np(l2)]) if n1 else _np(l2)
    print(f"256 states {optimizer} n_iter {n_iter} {'whole word' if full_word else f'M {M}'}: loss max rel "
          f"{np.abs(loss / ref_loss - 1).max():.2e}; weights max |dw| "
          f"{max(float(np.abs(_np(p) - ref_w[i]).max()) for i, p in enumerate(det.net.parameters())):.2e}")
    assert np.allclose(loss, ref_loss, rtol=2e-4, atol=1e-6)
    for i, p in enumerate(det.net.parameters()):
        assert np.all(np.abs(_np(p) - ref_w[i]) <= 2e-5 + 1e-3 * np.abs(ref_w[i])), i
    if optimizer == "SGD":  # (torch.optim.SGD keeps no state: the kernel leaves the moments alone)
        assert not tr.exp_avg.any() and not tr.exp_avg_sq.any()
