"""GPU: lstm_train_kernel's gradient, element by element, against torch autograd in float64 at the kernel's loop edges
(tests/lstm_grad_cases.py: the readout through Adam's first moment, the case table, the bound measured from stock float32 torch),
and mvn_lstm_train_f32's padded rows and word order through the raw ABI.  What tests/test_gpu_lstm_train.py cannot see: Adam and
RMSprop divide the gradient's scale out, its SGD case is checked by norm, its draws have no duplicates and its rows no padding.

tools/lstm_train_gradients.py prints the kernel's error in units of max(d32, floor) per case and tensor; the margin
of 8 is the one lstm_grad_cases derives, not one fitted to the kernel."""
import numpy as np
import pytest
import torch

import lstm_grad_cases as G
import meta_viterbinet_amd as mvn
from test_lstm_train_host import default_init_weights, detector_with

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_kernel_gradient_per_element(name):
    """|g - g64| <= 8 max(d32, floor) for every element of the ten tensors, exact zeros where the referee has them, b_ih = b_hh
    bitwise, the loss, exp_avg_sq to 4 ulp and the SGD step to 1 ulp."""
    G.check_first_iteration(G.CASES[name], DEV, True, G.MARGIN_KERNEL)


@pytest.mark.parametrize("name", G.SECOND_NAMES)
def test_kernel_second_iteration_gradient(name):
    """After a step that moved every weight by a third of its scale: the gradient of iteration 2 alone, at the kernel's own
    weights (the column copies and the fc layer every workgroup re-reads between iterations)."""
    G.check_second_iteration(G.CASES[name], DEV, True, G.MARGIN_KERNEL)


def test_permutation_of_all_positions_is_the_whole_word():
    """M = 256 distinct positions of T = 256: every count is 1 and the scale 1 / 256 both ways, so parameters, moments and loss are
    those of the whole word, bit for bit."""
    a = G.run(G.CASES["perm_T256_M256"], DEV, True)
    b = G.run(G.CASES["whole_T256"], DEV, True)
    assert _bits_equal(a["w"] + a["m"] + a["v"] + [a["loss"]], b["w"] + b["m"] + b["v"] + [b["loss"]])


@pytest.mark.parametrize("M", [8, 0])
def test_raw_abi_padded_rows_and_word_order(M):
    """mvn_lstm_train_f32 itself with y_ld = T + 5 and bits_ld = T + 3 (NaN and 7 in the padding), word_of_iter = [2, 0, 2, 1] over
    three words and positions drawn with one duplicate per row: bit-identical to LSTMOnlineTrainer.train_words on the compact rows
    [2, 0, 2, 1] (which always passes y_ld = bits_ld = T and word_of_iter = arange)."""
    T, n_words, n_iter = 37, 3, 4
    y_ld, bits_ld = T + 5, T + 3
    order = [2, 0, 2, 1]
    rng = np.random.RandomState(37)
    bits = rng.randint(0, 2, (n_words, T))
    rx = ((1 - 2 * bits) + 0.4 * rng.randn(n_words, T)).astype(np.float32)
    idx = None
    if M:
        rows = [rng.permutation(np.arange(1, T - 1))[:M - 1] for _ in range(n_iter)]
        rows[0][0], rows[1][0] = T - 1, 0  # both ends of the word are drawn
        idx = torch.from_numpy(np.stack([np.append(r, r[2]) for r in rows]).astype(np.int32))  # one position twice per row
        assert all(len(set(r.tolist())) == M - 1 for r in idx)
    ws = default_init_weights(3)
    # through the trainer, on compact rows in the order of the iterations
    tr = mvn.LSTMOnlineTrainer(detector_with(ws, DEV), use_kernel=True)
    assert tr.kernel_route(T)
    loss = tr.train_words(torch.from_numpy(bits[order].astype(np.float32)).to(DEV), torch.from_numpy(rx[order]).to(DEV), batch_idx=idx,
                          full_word=idx is None, return_loss=True)
    tr.check_status()
    want = [p.detach().cpu().numpy() for p in tr.params] + [tr.exp_avg.cpu().numpy(), tr.exp_avg_sq.cpu().numpy(), loss.cpu().numpy()]
    # through the ABI, on padded rows in storage order
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    y_pad = np.full((n_words, y_ld), np.nan, np.float32)
    y_pad[:, :T] = rx
    bits_pad = np.full((n_words, bits_ld), 7, np.int32)
    bits_pad[:, :T] = bits
    y_d, bits_d = torch.from_numpy(y_pad).to(DEV), torch.from_numpy(bits_pad).to(DEV)
    woi = torch.tensor(order, dtype=torch.int32, device=DEV)
    idx_d = None if idx is None else idx.to(DEV).contiguous()
    p = [torch.from_numpy(w.copy()).to(DEV) for w in ws]
    m, v = torch.zeros(int(G.OFFSETS[-1]), device=DEV), torch.zeros(int(G.OFFSETS[-1]), device=DEV)
    loss_d = torch.full((n_iter,), float("nan"), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.mvn_lstm_train_workspace_bytes(T))
    wsp = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    with mvn._lib.on_device(DEV):
        rc = lib.mvn_lstm_train_f32(ptr(y_d), y_ld, ptr(bits_d), bits_ld, n_words, ptr(woi), ptr(idx_d), M, n_iter, *[ptr(t) for t in p],
                                    ptr(m), ptr(v), 0, 1e-3, 0.9, 0.999, 1e-8, ptr(loss_d), ptr(wsp), ws_bytes, ptr(status), T,
                                    mvn._lib.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = [t.cpu().numpy() for t in p] + [m.cpu().numpy(), v.cpu().numpy(), loss_d.cpu().numpy()]
    assert np.isfinite(got[-1]).all() and all(np.isfinite(a).all() for a in got[:10])
    assert _bits_equal(got, want)
