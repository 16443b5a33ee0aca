"""GPU: first-order online meta-learning of the LSTM detector in one launch (lstm_maml_kernel behind mvn_lstm_maml_train_f32,
LSTMMetaTrainer.maml_training) -- bitwise against the pinned training kernel where the two must agree (meta_lr = 0), theta kept
apart from theta' (outer lr = 0), the meta-gradient element by element against float64 through Adam's first moment
(tests/lstm_grad_cases.py's readout and bound), whole steps against the float64 referee of tests/test_lstm_meta_host.py with the
project's training bounds (2e-5 + 1e-3 |w| on parameters, rtol 2e-4 on the loss), split calls and padded rows through the raw ABI,
the second-order autograd route, and golden G20 through the harness."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_grad_cases as G
import meta_viterbinet_amd as mvn
from test_lstm_host import g18_weights
from test_lstm_meta_host import (check_g20_by_word, g20_by_word, meta_gradients, meta_referee, run_g20_part, run_meta, words)
from test_lstm_train_host import check_g19_part, check_losses, default_init_weights, detector_with, outside

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META_LR = 0.1


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lstm")


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_lstm_meta")


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _state(tr, loss):
    return [p.detach().cpu().numpy() for p in tr.params] + [tr.exp_avg.cpu().numpy(), tr.exp_avg_sq.cpu().numpy(), np.asarray(loss)]


def _dev(bits, rx):
    return torch.from_numpy(bits.astype(np.float32)).to(DEV), torch.from_numpy(rx).to(DEV)


def test_meta_lr_zero_is_the_pinned_training_kernel():
    """meta_lr = 0: theta' = theta, so a meta step is one whole-word iteration of lstm_train_kernel on the query word -- parameters,
    both moments and the losses bit for bit, whatever the support word was."""
    T, sup, qry = 37, [[3], [0], [2]], [1, 2, 0]
    ws = default_init_weights(3)
    bits, rx = words(T, 4)
    _, loss, tr = run_meta(ws, bits, rx, sup, qry, 0.0, False, DEV, True)
    assert tr.meta_kernel_route(T, 1, False) and tr.step == 3
    ref = mvn.LSTMOnlineTrainer(detector_with(ws, DEV), use_kernel=True)
    tx_d, rx_d = _dev(bits, rx)
    ref_loss = ref.train_words(tx_d[qry], rx_d[qry], full_word=True, return_loss=True)
    ref.check_status()
    assert np.isfinite(loss).all()
    assert _bits_equal(_state(tr, loss), _state(ref, ref_loss.cpu().numpy()))


def test_outer_lr_zero_leaves_theta_alone_and_the_loss_is_taken_at_the_fast_weights():
    """Outer lr = 0, meta_lr = 0.1: the inner step must never reach a.w[] -- every parameter bitwise unchanged over 3 steps -- while
    loss_out is the query loss at theta' (float64, rtol 2e-4), not at theta."""
    T, sup, qry = 37, [[0], [1], [3]], [1, 2, 0]
    ws = default_init_weights(3)
    bits, rx = words(T, 4)
    got, loss, tr = run_meta(ws, bits, rx, sup, qry, META_LR, False, DEV, True, lr=0.0)
    assert _bits_equal(got, ws)
    want, at_theta = [], []
    for s, q in zip(sup, qry):
        want.append(meta_gradients(ws, bits, rx, s, q, META_LR, torch.float64)[1])
        at_theta.append(meta_gradients(ws, bits, rx, s, q, 0.0, torch.float64)[1])
    print("query loss at theta'", want, "at theta", at_theta, "kernel", loss.tolist())
    assert np.all(np.abs(np.array(want) - np.array(at_theta)) > 1e-3 * np.array(want))  # the test can tell the two apart
    check_losses(loss, np.array(want))
    assert tr.exp_avg.any()  # (the optimizer ran: lr = 0 only hides its step)


_META_REF = {}


def _meta_reference(T, same):
    """The float64 meta-gradient of one step (support word 0, query word 1, or the same word twice) and stock float32 torch's
    distance from it on the same two-stage computation; computed once per case."""
    if (T, same) not in _META_REF:
        ws = G.weights("init")
        bits, rx = words(T, 2)
        s, q = (1, 1) if same else (0, 1)
        g64, loss64, _ = meta_gradients(ws, bits, rx, [s], q, META_LR, torch.float64)
        g32, _, _ = meta_gradients(ws, bits, rx, [s], q, META_LR, torch.float32)
        _META_REF[(T, same)] = dict(g64=g64, loss64=loss64, d32=np.array([np.abs(a - b).max() for a, b in zip(g32, g64)]),
                                    floor=np.array([2.0 ** -23 * np.abs(b).max() for b in g64]), s=s, q=q, bits=bits, rx=rx, ws=ws)
    return _META_REF[(T, same)]


@pytest.mark.parametrize("T,same", [(1, False), (2, False), (5, False), (37, False), (136, False), (256, False), (37, True)])
def test_meta_gradient_per_element(T, same):
    """From a zero optimizer state one step with beta1 = 0.5 leaves exp_avg = g / 2: the first-order meta-gradient itself, for all
    795 138 parameters, against the float64 gradient of the query loss at fl64(theta - meta_lr grad L_s(theta)).  Bound
    (tests/lstm_grad_cases.py): 8 max(d32, 2^-23 max |g64|) per tensor, d32 stock float32 torch's error on the same computation.
    T = 1, 2: the skew guards; 5: Tp padding; 256: the LDS edge; same: support word == query word."""
    ref = _meta_reference(T, same)
    _, loss, tr = run_meta(ref["ws"], ref["bits"], ref["rx"], [[ref["s"]]], [ref["q"]], META_LR, False, DEV, True, lr=G.LR, betas=G.BETAS)
    assert tr.meta_kernel_route(T, 1, False) and tr.step == 1
    g = [np.float32(2.0) * m for m in G.split(tr.exp_avg)]
    G.compare(f"meta_T{T}{'_same' if same else ''}", g, ref, G.MARGIN_KERNEL)
    check_losses(loss, np.array([ref["loss64"]]))
    for bi, bh in ((2, 3), (6, 7)):  # b_ih and b_hh of a layer share one gradient
        assert np.array_equal(g[bi].view(np.uint32), g[bh].view(np.uint32))


@pytest.mark.parametrize("optimizer_type,lr", [("Adam", 1e-3), ("RMSprop", 1e-3), ("SGD", 0.05)])
@pytest.mark.parametrize("T", [136, 256])
def test_four_steps_against_float64_autograd(T, optimizer_type, lr):
    """4 steps (support word k, query word k + 1) against meta_train_loop in float64 with torch.optim."""
    ws = default_init_weights(3)
    bits, rx = words(T, 5)
    sup, qry = [[0], [1], [2], [3]], [1, 2, 3, 4]
    got, loss, tr = run_meta(ws, bits, rx, sup, qry, META_LR, False, DEV, True, optimizer_type=optimizer_type, lr=lr)
    assert tr.meta_kernel_route(T, 1, False) and tr.step == 4
    ref_w, ref_loss = meta_referee(ws, bits, rx, sup, qry, META_LR, False, optimizer_type, lr)
    n_out, worst = outside(got, ref_w)
    print(f"T {T} {optimizer_type}: {n_out} parameters outside the bound, largest deviation {worst:.3g}")
    assert n_out == 0
    check_losses(loss, ref_loss)


def test_split_calls_and_padded_rows_through_the_raw_abi():
    """5 steps in one call equal 2 + 3 in two, bit for bit; and mvn_lstm_maml_train_f32 itself with rx_ld = T + 5 and
    bits_ld = T + 3 (NaN and 7 in the padding) gives the same bits as the trainer on compact rows."""
    T, n_words = 37, 4
    sup, qry = [[0], [1], [3], [2], [1]], [1, 2, 0, 3, 1]
    ws = default_init_weights(3)
    bits, rx = words(T, n_words)
    _, loss, tr = run_meta(ws, bits, rx, sup, qry, META_LR, False, DEV, True)
    want = _state(tr, loss)
    two = mvn.LSTMMetaTrainer(detector_with(ws, DEV), use_kernel=True)
    tx_d, rx_d = _dev(bits, rx)
    l1 = two.maml_training(rx_d, tx_d, torch.tensor(sup[:2]), torch.tensor(qry[:2]), META_LR, MAML=False, return_loss=True)
    l2 = two.maml_training(rx_d, tx_d, torch.tensor(sup[2:]), torch.tensor(qry[2:]), META_LR, MAML=False, return_loss=True)
    two.check_status()
    assert two.step == 5
    assert _bits_equal(_state(two, torch.cat([l1, l2]).cpu().numpy()), want)
    # the ABI on padded rows
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    rx_ld, bits_ld, n = T + 5, T + 3, len(qry)
    y_pad = np.full((n_words, rx_ld), np.nan, np.float32)
    y_pad[:, :T] = rx
    bits_pad = np.full((n_words, bits_ld), 7, np.int32)
    bits_pad[:, :T] = bits
    y_d, bits_d = torch.from_numpy(y_pad).to(DEV), torch.from_numpy(bits_pad).to(DEV)
    sup_d = torch.tensor(sup, dtype=torch.int32, device=DEV).reshape(-1).contiguous()
    qry_d = torch.tensor(qry, dtype=torch.int32, device=DEV)
    p = [torch.from_numpy(w.copy()).to(DEV) for w in ws]
    m, v = torch.zeros(int(G.OFFSETS[-1]), device=DEV), torch.zeros(int(G.OFFSETS[-1]), device=DEV)
    loss_d = torch.full((n,), float("nan"), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.mvn_lstm_maml_workspace_bytes(T))
    wsp = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    with mvn._lib.on_device(DEV):
        rc = lib.mvn_lstm_maml_train_f32(ptr(y_d), rx_ld, ptr(bits_d), bits_ld, n_words, ptr(sup_d), ptr(qry_d), n, *[ptr(t) for t in p],
                                         ptr(m), ptr(v), 0, META_LR, 1e-3, 0.9, 0.999, 1e-8, ptr(loss_d), ptr(wsp), ws_bytes, ptr(status), T,
                                         mvn._lib.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = [t.cpu().numpy() for t in p] + [m.cpu().numpy(), v.cpu().numpy(), loss_d.cpu().numpy()]
    assert all(np.isfinite(a).all() for a in got)
    assert _bits_equal(got, want)


def test_second_order_takes_autograd_on_the_gpu():
    """MAML=True is not built on the device: the trainer differentiates twice through MetaLSTMDetector on the GPU; against the CPU's
    float64 double backward."""
    T = 8
    ws = default_init_weights(3)
    bits, rx = words(T, 3)
    sup, qry = [[0], [1]], [1, 2]
    got, loss, tr = run_meta(ws, bits, rx, sup, qry, META_LR, True, DEV, True)
    assert not tr.meta_kernel_route(T, 1, True) and tr.step == 2
    ref_w, ref_loss = meta_referee(ws, bits, rx, sup, qry, META_LR, True)
    assert outside(got, ref_w)[0] == 0
    check_losses(loss, ref_loss)
    first_w, _ = meta_referee(ws, bits, rx, sup, qry, META_LR, False)
    assert outside(got, first_w)[0] > 0  # (the second-order term is visible at this bound)


def test_g20_first_order_meta_train_loop_through_the_kernel(g20, g18):
    got, losses, tr = run_g20_part(g20, g18, "b", DEV, use_kernel=True)
    assert tr.meta_kernel_route(136, 1, False)
    check_g19_part(g20, "b", got, losses)


@pytest.mark.parametrize("use_kernel", [True, False])
def test_g20_by_word_meta_update_branch(g20, g18, use_kernel):
    """The reference's evaluate() by word with online_meta, first order: the same ser outside the blocks exempt by margin, the same
    blocks trained and meta-updated, the final weights within the digest bound -- every meta update ONE maml_training call."""
    det = detector_with(g18_weights(g18), DEV)
    tr = mvn.LSTMMetaTrainer(det, use_kernel=use_kernel)
    assert tr.meta_kernel_route(136, 1, False) == use_kernel
    ser, trained, metas = g20_by_word(g20, det, tr, DEV)
    check_g20_by_word(g20, ser, trained, metas, [p.detach().cpu().numpy() for p in tr.params])
    assert tr.step == sum(len(np.unique(r)) for r in g20["c_randint"]) + int(g20["c_meta"][0]) * len(trained)


def test_kernel_name_and_arguments_on_the_device():
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    buf = ctypes.create_string_buffer(128)
    assert lib.mvn_lstm_maml_kernel_name(136, buf, 128) == 0 and b"lstm_maml_kernel x 64" in buf.value
    assert lib.mvn_lstm_maml_kernel_name(257, buf, 128) == -1
    T = 5
    t = torch.zeros(1024 * 256, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.mvn_lstm_maml_workspace_bytes(T))
    wsp = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def call(n_steps=1, wsb=ws_bytes, sup=i, T=T):
        return lib.mvn_lstm_maml_train_f32(ptr(t), 8, ptr(i), 8, 1, ptr(sup), ptr(i), n_steps, *([ptr(t)] * 10), ptr(t), ptr(t), 0, 0.1, 1e-3,
                                           0.9, 0.999, 1e-8, None, ptr(wsp), wsb, None, T, mvn._lib.current_stream(DEV))

    assert call(n_steps=0) == 0 and call(n_steps=-1) == -1 and call(T=9) == -1
    assert call(wsb=int(lib.mvn_lstm_train_workspace_bytes(T))) == -5  # the training workspace has no room for the fast weights
    assert call(sup=None) == -4
