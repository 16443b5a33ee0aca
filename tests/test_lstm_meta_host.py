"""CPU-only: online meta-learning of the LSTM detector (meta-viterbinet_amd/lstm.py: LSTMMetaTrainer; the meta-learning form of
lstm_train_kernel behind mvn_lstm_maml_train_f32 on the GPU).  The C ABI's argument checks without a device, the new kernel's
resources in the gfx950 code object, the autograd route against golden G20 (tests/golden/make_golden_lstm_meta.py) within the bounds
G19 is held to, maml_training's index semantics, the optimizer state shared with online_training, and the harness's refusals.

The float64 referee (meta_referee) is the reference's meta_train_loop on MetaLSTMDetector in float64 with torch.optim; the helpers
are shared with tests/test_gpu_lstm_meta.py."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L
from test_lstm_host import g18_weights
from test_lstm_train_host import cpu_rs  # noqa: F401  (fixture: the harness's Reed-Solomon calls on the CPU oracle)
from test_lstm_train_host import (_cpu_val_detector, check_digest, check_g19_by_word, check_g19_part, check_losses,
                                  default_init_weights, detector_with, outside)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_lstm_meta.py
# ---------------------------------------------------------------------------------------------------------------------------
def words(T, n, seed=None):
    """n words seeded by T: (bits int64 [n, T], rx float32 [n, T])."""
    rng = np.random.RandomState(1000 + T if seed is None else seed)
    bits = rng.randint(0, 2, (n, T))
    rx = ((1 - 2 * bits) + 0.4 * rng.randn(n, T)).astype(np.float32)
    return bits, rx


def meta_gradients(ws, bits, rx, s, q, meta_lr, dtype, MAML=False):
    """One meta_train_loop (trainer.py:425-453) up to the optimizer on the CPU in `dtype`: (meta-gradient as ten float64 arrays, query
    loss, support gradient).  First order: the gradient of the query loss at fl(theta - meta_lr grad L_s(theta))."""
    params = [torch.from_numpy(np.asarray(w)).to(dtype).requires_grad_() for w in ws]
    y, lab = torch.from_numpy(np.asarray(rx)).to(dtype), torch.from_numpy(np.asarray(bits)).long()
    det = L.MetaLSTMDetector()
    s = torch.as_tensor(s).reshape(-1).long()
    loss_s = torch.nn.functional.cross_entropy(det(y[s], "train", params).reshape(-1, 2), lab[s].reshape(-1))
    g_s = torch.autograd.grad(loss_s, params, create_graph=MAML)
    updated = [p - meta_lr * g for g, p in zip(g_s, params)]
    loss_q = torch.nn.functional.cross_entropy(det(y[q:q + 1], "train", updated).reshape(-1, 2), lab[q])
    g_q = torch.autograd.grad(loss_q, params)
    return [g.double().numpy() for g in g_q], float(loss_q.detach()), [g.detach().double().numpy() for g in g_s]


def meta_referee(ws, bits, rx, sup, qry, meta_lr, MAML, optimizer_type="Adam", lr=1e-3):
    """n meta-learning steps in float64 with torch.optim: (final weights as float64 arrays, query losses [n])."""
    params = [torch.from_numpy(np.asarray(w)).double().requires_grad_() for w in ws]
    opt = {"Adam": torch.optim.Adam, "RMSprop": torch.optim.RMSprop, "SGD": torch.optim.SGD}[optimizer_type](params, lr=lr)
    y, lab = torch.from_numpy(np.asarray(rx)).double(), torch.from_numpy(np.asarray(bits)).long()
    det = L.MetaLSTMDetector()
    sup = np.asarray(sup).reshape(len(qry), -1)
    losses = []
    for s, q in zip(sup, np.asarray(qry)):
        s = torch.as_tensor(s).long()
        loss_s = torch.nn.functional.cross_entropy(det(y[s], "train", params).reshape(-1, 2), lab[s].reshape(-1))
        g_s = torch.autograd.grad(loss_s, params, create_graph=MAML)
        updated = [p - meta_lr * g for g, p in zip(g_s, params)]
        loss_q = torch.nn.functional.cross_entropy(det(y[[int(q)]], "train", updated).reshape(-1, 2), lab[int(q)])
        grads = torch.autograd.grad(loss_q, params)
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
        losses.append(float(loss_q.detach()))
    return [p.detach().numpy().copy() for p in params], np.array(losses)


def run_meta(ws, bits, rx, sup, qry, meta_lr, MAML, device, use_kernel, optimizer_type="Adam", lr=1e-3, betas=(0.9, 0.999)):
    """The steps through LSTMMetaTrainer.maml_training: (final weights, query losses, trainer)."""
    det = detector_with(ws, device)
    tr = mvn.LSTMMetaTrainer(det, lr=lr, betas=betas, use_kernel=use_kernel, optimizer_type=optimizer_type)
    loss = tr.maml_training(torch.from_numpy(np.asarray(rx)).to(device), torch.from_numpy(np.asarray(bits, np.float32)).to(device),
                            torch.as_tensor(np.asarray(sup)), torch.as_tensor(np.asarray(qry)), meta_lr, MAML, return_loss=True)
    tr.check_status()
    return [p.detach().cpu().numpy() for p in tr.params], loss.cpu().numpy(), tr


def run_g20_part(g20, g18, part, device, use_kernel):
    """G20 (a) / (b): 4 steps, support word w and query word w + 1."""
    return run_meta(g18_weights(g18), g20["a_tx"], g20["a_rx"], [[0], [1], [2], [3]], [1, 2, 3, 4], 0.1, part == "a", device, use_kernel)


class ReplayJHat:
    """The `draws` of eval_by_word that replays the recorded torch.randint draws of trainer.py:337 in call order."""

    def __init__(self, high, values):
        self.high, self.values, self.at = np.asarray(high), np.asarray(values), 0

    def j_hat_update(self, high, iterations, size):
        rows = self.values[self.at:self.at + iterations]
        assert rows.shape == (iterations, size) and np.all(self.high[self.at:self.at + iterations] == high)  # the same buffer length
        self.at += iterations
        return np.concatenate([np.unique(r) for r in rows])  # torch.unique(torch.randint(...))

    def j_hat(self, high, size):
        return self.j_hat_update(high, 1, size)


def g20_by_word(g20, detector, trainer, device):
    """G20 (c) through mvn.eval_by_word: (ser_by_word, blocks that trained, blocks with a meta update)."""
    ss_iters, sub, nsym, snr, _, meta_iters, meta_j, meta_sub = [int(v) for v in g20["c_meta"]]
    tx = torch.from_numpy(g20["c_tx"].astype(np.float32)).to(device)
    rx = torch.from_numpy(g20["c_rx"]).to(device)
    draws = ReplayJHat(g20["c_randint_high"], g20["c_randint"])
    trained, metas = [], []

    def observer(seen):
        if seen["stage"] == "end" and seen["trained"]:
            trained.append(seen["count"])
        if seen["stage"] == "meta":
            metas.append(seen["count"])

    ser = mvn.eval_by_word(detector, tx, rx, float(snr), 0.2, n_symbols=nsym, subframes_in_frame=sub, self_supervised=True,
                           online_trainer=trainer, self_supervised_iterations=ss_iters, ser_thresh=float(g20["c_ser_thresh"]),
                           online_meta=True, meta_lr=float(g20["c_meta_lr"]), MAML=False, window_size=1,
                           meta_train_iterations=meta_iters, meta_j_num=meta_j, meta_subframes=meta_sub,
                           meta_style_online_training=True, weights_init="last_frame", draws=draws, observer=observer)
    assert draws.at == len(g20["c_randint"]) or metas != list(g20["c_meta_blocks"])
    return ser, trained, metas


def check_g20_by_word(g20, ser, trained, metas, weights):
    """G19's by-word comparison (ser equal outside the blocks exempt by margin, the same blocks trained), the same blocks
    meta-updated, and the final weights within the digest bound."""
    assert len(g20["c_meta_blocks"]) >= 3 and len(g20["c_trained"]) >= 5
    assert metas == [int(b) for b in g20["c_meta_blocks"]]
    check_g19_by_word(g20, ser, trained)
    check_digest(weights, g20, "c_")


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lstm")


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_lstm_meta")


def test_symbols_bound_and_validation():
    lib = mvn._lib.load()
    for name in ("mvn_lstm_maml_workspace_bytes", "mvn_lstm_maml_train_f32", "mvn_lstm_maml_kernel_name"):
        assert name in mvn._lib.SIGNATURES and hasattr(lib, name)
    assert lib.mvn_version() == 6
    ws = lib.mvn_lstm_maml_workspace_bytes(136)
    assert ws == lib.mvn_lstm_train_workspace_bytes(136) + (3 * 1024 * 256 + 514 + 2) * 4  # the fast-weight image, padded to 16 bytes
    assert lib.mvn_lstm_maml_workspace_bytes(0) == 0 and lib.mvn_lstm_maml_workspace_bytes(257) == 0
    fake = ctypes.c_void_p(4096)  # never dereferenced: every check below happens before a device call

    def call(T=136, rx_ld=136, bits_ld=136, n_words=3, n_steps=5, ptr=fake, sup=fake, qry=fake, wsp=fake, wsb=ws, step0=0):
        return lib.mvn_lstm_maml_train_f32(ptr, rx_ld, ptr, bits_ld, n_words, sup, qry, n_steps, *([ptr] * 10), ptr, ptr, step0, 0.1, 1e-3,
                                           0.9, 0.999, 1e-8, None, wsp, wsb, None, T, None)

    assert call(T=0) == -1
    assert call(T=257, rx_ld=300, bits_ld=300) == -1  # above MVN_LSTM_TRAIN_MAX_T
    assert call(rx_ld=135) == -1 and call(bits_ld=135) == -1
    assert call(n_steps=-1) == -1 and call(n_words=0) == -1 and call(step0=-1) == -1
    assert call(T=0, ptr=None) == -1  # shapes before pointers
    assert call(n_steps=0, ptr=None, wsp=None) == 0  # a no-op
    assert call(ptr=None) == -4 and call(wsp=None) == -4 and call(sup=None) == -4 and call(qry=None) == -4
    assert call(wsb=ws - 4) == -5 and call(wsb=lib.mvn_lstm_train_workspace_bytes(136)) == -5
    assert call(wsp=ctypes.c_void_p(4100)) == -5  # 16-byte alignment
    buf = ctypes.create_string_buffer(128)
    assert lib.mvn_lstm_maml_kernel_name(136, buf, 128) == 0 and b"lstm_maml_kernel" in buf.value and b"first order" in buf.value
    assert lib.mvn_lstm_maml_kernel_name(257, buf, 128) == -1 and lib.mvn_lstm_maml_kernel_name(0, buf, 128) == -1
    assert lib.mvn_lstm_maml_kernel_name(136, None, 128) == -4


def test_kernels_in_code_object_no_scratch():
    """lstm_maml_kernel is in the gfx950 code object beside lstm_train_kernel, neither spills, the meta-learning form takes no more
    static LDS than the training kernel (its dynamic LDS is the same LtLds), and lstm_train_kernel holds no more than the 465 VGPRs
    it had before the two shared one body."""
    import tempfile

    import __graft_entry__ as g

    so = g.build_hip()
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    bundler, readelf = os.path.join(llvm, "clang-offload-bundler"), os.path.join(llvm, "llvm-readelf")
    assert os.path.exists(bundler) and os.path.exists(readelf) and shutil.which("c++filt")
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, elf = os.path.join(tmp, "fatbin"), os.path.join(tmp, "dev.elf")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, so, os.path.join(tmp, "unused")],
                       check=True)
        subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fatbin, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--output=" + elf], check=True)
        notes = subprocess.run([readelf, "--notes", elf], check=True, capture_output=True, text=True).stdout
    table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], input=notes, check=True,
                           capture_output=True, text=True).stdout
    rows = [re.match(r"(.+?)\s+vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) static_lds (\d+)$", ln) for ln in table.splitlines()]
    rows = {m.group(1): m for m in rows if m}
    assert "lstm_train_kernel" in rows and "lstm_maml_kernel" in rows
    train, maml = rows["lstm_train_kernel"], rows["lstm_maml_kernel"]
    print(f"lstm_train_kernel: {train.group(2)} VGPRs, scratch {train.group(4)}; lstm_maml_kernel: {maml.group(2)} VGPRs, scratch {maml.group(4)}")
    assert int(train.group(4)) == 0 and int(maml.group(4)) == 0
    assert int(train.group(2)) <= 465
    assert int(maml.group(5)) == int(train.group(5))
    assert int(maml.group(5)) + mvn._lib.load().mvn_lstm_train_lds_bytes(256) <= 160 * 1024


@pytest.mark.parametrize("part", ["a", "b"])
def test_g20_meta_train_loop_autograd_route(g20, g18, part):
    """(a) second order, (b) first order: query losses and the weight digest of the reference's four meta_train_loop calls."""
    got, losses, tr = run_g20_part(g20, g18, part, "cpu", use_kernel=False)
    assert tr.step == 4 and not tr.meta_kernel_route(136, 1, part == "a")
    check_g19_part(g20, part, got, losses)


def test_g20_by_word_cpu_route(g20, g18, cpu_rs):  # noqa: F811
    det = _cpu_val_detector(g18_weights(g18))
    tr = mvn.LSTMMetaTrainer(det, use_kernel=False)
    ser, trained, metas = g20_by_word(g20, det, tr, "cpu")
    check_g20_by_word(g20, ser, trained, metas, [p.detach().numpy() for p in tr.params])


def test_negative_and_repeated_indices_two_support_words_and_losses():
    """support_idx [n, W] / query_idx [n] index the buffer like the reference's fancy indexing: negative entries count from the end,
    a word may serve twice, W = 2 support words give one loss over both; return_loss returns the n query losses."""
    T, Nw = 6, 4
    ws = default_init_weights(3)
    bits, rx = words(T, Nw)
    sup, qry = [[-3, -2], [0, 0], [-4, 1]], [-1, 0, -2]
    a_w, a_loss, a_tr = run_meta(ws, bits, rx, sup, qry, 0.1, True, "cpu", True)  # a CPU detector takes autograd whatever use_kernel says
    b_w, b_loss, _ = run_meta(ws, bits, rx, [[1, 2], [0, 0], [0, 1]], [3, 0, 2], 0.1, True, "cpu", False)
    assert all(np.array_equal(x, y) for x, y in zip(a_w, b_w)) and np.array_equal(a_loss, b_loss)
    assert a_loss.shape == (3,) and a_loss.dtype == np.float32 and a_tr.step == 3
    ref_w, ref_loss = meta_referee(ws, bits, rx, [[1, 2], [0, 0], [0, 1]], [3, 0, 2], 0.1, True)
    assert outside(a_w, ref_w)[0] == 0
    check_losses(a_loss, ref_loss)
    det = detector_with(ws)
    tr = mvn.LSTMMetaTrainer(det, use_kernel=False)
    assert tr.maml_training(torch.from_numpy(rx), torch.from_numpy(bits.astype(np.float32)), torch.tensor(sup), torch.tensor(qry), 0.1) is None
    assert all(np.array_equal(p.detach().numpy(), w) for p, w in zip(tr.params, a_w))
    # first order differs from second order, and both are what the referee says
    c_w, c_loss, _ = run_meta(ws, bits, rx, sup, qry, 0.1, False, "cpu", False)
    assert not all(np.array_equal(x, y) for x, y in zip(a_w, c_w))
    ref_w, ref_loss = meta_referee(ws, bits, rx, [[1, 2], [0, 0], [0, 1]], [3, 0, 2], 0.1, False)
    assert outside(c_w, ref_w)[0] == 0
    check_losses(c_loss, ref_loss)


def test_optimizer_state_runs_through_online_and_meta_training():
    """One optimizer (trainer.py:163-175, :452, :503): online_training and maml_training share exp_avg, exp_avg_sq and step."""
    T = 6
    ws = default_init_weights(3)
    bits, rx = words(T, 3)
    tx_t, rx_t = torch.from_numpy(bits.astype(np.float32)), torch.from_numpy(rx)
    tr = mvn.LSTMMetaTrainer(detector_with(ws), use_kernel=False)
    tr.online_training(tx_t[:1], rx_t[:1], iterations=2, full_word=True)
    assert tr.step == 2
    m2 = tr.exp_avg.clone()
    tr.maml_training(rx_t, tx_t, torch.tensor([[0], [1]]), torch.tensor([1, 2]), 0.1, MAML=False)
    assert tr.step == 4 and not torch.equal(m2, tr.exp_avg)
    tr.online_training(tx_t[2:], rx_t[2:], iterations=1, full_word=True)
    assert tr.step == 5
    # the same five steps on torch.optim.Adam in float64
    params = [torch.from_numpy(w).double().requires_grad_() for w in ws]
    opt = torch.optim.Adam(params, lr=1e-3)
    y, lab, det = rx_t.double(), torch.from_numpy(bits).long(), L.MetaLSTMDetector()
    ce = torch.nn.functional.cross_entropy

    def step(grads):
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()

    for _ in range(2):
        step(torch.autograd.grad(ce(det(y[:1], "train", params).reshape(-1, 2), lab[0]), params))
    for s, q in ((0, 1), (1, 2)):
        g_s = torch.autograd.grad(ce(det(y[s:s + 1], "train", params).reshape(-1, 2), lab[s]), params)
        upd = [p - 0.1 * g for g, p in zip(g_s, params)]
        step(torch.autograd.grad(ce(det(y[q:q + 1], "train", upd).reshape(-1, 2), lab[q]), params))
    step(torch.autograd.grad(ce(det(y[2:], "train", params).reshape(-1, 2), lab[2]), params))
    assert outside([p.detach().numpy() for p in tr.params], [p.detach().numpy() for p in params])[0] == 0
    m_ref = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params])
    assert float((tr.exp_avg.double() - m_ref).abs().max()) <= 1e-5 * float(m_ref.abs().max())
    tr.reset_state()
    assert tr.step == 0 and not tr.exp_avg.any()


def test_routes_and_refusals(g18):
    ws = g18_weights(g18)
    det = _cpu_val_detector(ws)
    tr = mvn.LSTMMetaTrainer(det)
    assert isinstance(tr, mvn.LSTMOnlineTrainer) and tr.optimizer_type == "Adam" and tr.step == 0
    assert not tr.meta_kernel_route(136, 1, False)  # a CPU detector
    for T, W, MAML in ((136, 1, True), (136, 2, False), (257, 1, False), (0, 1, False)):
        assert not tr.meta_kernel_route(T, W, MAML)
    with pytest.raises(NotImplementedError, match="LSTMMetaTrainer"):
        mvn.LSTMOnlineTrainer(det).maml_training()
    with pytest.raises(ValueError):
        mvn.LSTMMetaTrainer(mvn.VNETDetector(16, {"train": 8, "val": 8}))
    tx, rx = torch.zeros(3, 120), torch.zeros(3, 136)
    kw = dict(n_symbols=2, subframes_in_frame=25)
    with pytest.raises(ValueError, match="LSTMMetaTrainer"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, online_meta=True, online_trainer=mvn.LSTMOnlineTrainer(det), **kw)
    with pytest.raises(ValueError, match="LSTM"):
        mvn.eval_by_word(L.MetaLSTMDetector(), tx, rx, 10.0, 0.2, online_meta=True, online_trainer=tr, **kw)
    with pytest.raises(ValueError, match="LSTMMetaTrainer"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, online_meta=True, **kw)
    vdet = mvn.VNETDetector(16, {"train": 136, "val": 136})
    with pytest.raises(ValueError, match="LSTMOnlineTrainer"):
        mvn.eval_by_word(vdet, tx, rx, 10.0, 0.2, online_meta=True, online_trainer=tr, **kw)
    with pytest.raises(ValueError, match="weights init"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, online_meta=True, online_trainer=tr, weights_init="nonsense", **kw)


@pytest.mark.parametrize("weights_init", ["random", "meta_training"])
def test_by_word_weights_init(g18, g20, cpu_rs, weights_init):  # noqa: F811
    """'meta_training' restarts every meta update from the ten given arrays, 'random' from freshly drawn weights and a fresh
    optimizer (trainer.py:356-366): seen through the observer right after the first update's maml_training call."""
    ws = g18_weights(g18)
    det = _cpu_val_detector(ws)
    tr = mvn.LSTMMetaTrainer(det, use_kernel=False)
    tx, rx = torch.from_numpy(g20["c_tx"][:6].astype(np.float32)), torch.from_numpy(g20["c_rx"][:6])
    given = default_init_weights(5)
    seen = []
    tr.step = 7
    mvn.eval_by_word(det, tx, rx, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, online_meta=True, MAML=False,
                     online_trainer=tr, ser_thresh=1.0, meta_train_iterations=1, meta_j_num=1, meta_subframes=3,
                     weights_init=weights_init, meta_training_weights=given, observer=seen.append)
    metas = [s for s in seen if s["stage"] == "meta"]
    assert [s["count"] for s in metas] == [3]
    sup, qry = metas[0]["meta"]
    assert sup.shape == (1, 1) and qry.shape == (1,) and int(qry[0]) == int(sup[0, 0]) + 1
    if weights_init == "random":
        assert tr.step == 1  # a fresh optimizer, one step
        assert all(float((p.detach() - torch.from_numpy(w)).abs().max()) > 1e-2 for p, w in zip(tr.params[4:6], ws[4:6]))
    else:
        assert tr.step == 8
        start = detector_with(given)
        tr2 = mvn.LSTMMetaTrainer(start, use_kernel=False)
        tr2.step = 7
        tr2.maml_training(metas[0]["buffer_rx"], metas[0]["buffer_tx"], sup, qry, 0.1, MAML=False)
        assert all(torch.equal(a, b) for a, b in zip(tr.params, tr2.params))
