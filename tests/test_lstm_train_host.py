"""CPU-only: training of the LSTM detector (meta-viterbinet_amd/lstm.py: LSTMOnlineTrainer; csrc/lstm_train.inc behind
mvn_lstm_train_f32).  The C ABI's argument checks without a device, the kernel's resources in the gfx950 code object, the
autograd route (use_kernel=False, the CPU route) against torch autograd + torch.optim in float64, golden G19
(tests/golden/make_golden_lstm_train.py) and the harness's update branch with the refusals around it.

Tolerance (the project's training tests, tests/test_gpu_parity.py): parameters |d| <= 2e-5 + 1e-3 |w|, per-iteration loss
rtol 2e-4 / atol 1e-6, against the float64 referee started from identical weights and draws.  In the Adam cases more than 90 % of
the parameters move by more than ten times that bound, so it is a sensitive one; SGD's small updates are checked relative to the
update itself as well.  What it does not see -- Adam and RMSprop divide the gradient's scale out, so a gradient short of a time step
or wrong by a factor gives nearly the same update; one wrong row hides in a tensor's norm; no draw here repeats a position -- is
held element by element in tests/lstm_grad_cases.py (tests/test_lstm_grad_host.py, tests/test_gpu_lstm_grad.py): the gradient itself,
read out of Adam's first moment, at T = 1 ... 256."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS = 795138


# ---------------------------------------------------------------------------------------------------------------------------
# shared with tests/test_gpu_lstm_train.py
# ---------------------------------------------------------------------------------------------------------------------------
def default_init_weights(seed=3):
    """nn.LSTM / nn.Linear's default initialisation under torch.manual_seed(seed) (the global generator is left as it was)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        det = L.LSTMDetector()
        return [p.detach().cpu().numpy().copy() for p in det._params()]


def detector_with(ws, device="cpu"):
    with torch.random.fork_rng(devices=[]):
        det = L.LSTMDetector().to(device)
    det.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(device) for k, w in zip(det.state_dict().keys(), ws)})
    return det


def draw_batches(T, n, M, seed):
    """n minibatches like select_batch (trainer.py:542) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.multinomial(torch.arange(T, dtype=torch.float32).expand(n, T), M, generator=g).to(torch.int32)


def referee(ws, tx, rx, word_of_iter, idx, n, optimizer_type="Adam", lr=1e-3, state=None):
    """torch autograd + torch.optim in float64 on the CPU: n steps, step i on word word_of_iter[i] (None: word 0) with the loss over
    positions idx[i] (None: the whole word).  Returns (final weights as float64 arrays, losses [n], state to carry on with)."""
    if state is None:
        lstm = torch.nn.LSTM(L.INPUT_SIZE, L.HIDDEN_SIZE, L.NUM_LAYERS, batch_first=True).double()
        fc = torch.nn.Linear(L.HIDDEN_SIZE, L.N_CLASSES).double()
        params = list(lstm.parameters()) + list(fc.parameters())
        with torch.no_grad():
            for p, w in zip(params, ws):
                p.copy_(torch.from_numpy(np.asarray(w)).double())
        opt = {"Adam": torch.optim.Adam, "RMSprop": torch.optim.RMSprop, "SGD": torch.optim.SGD}[optimizer_type](params, lr=lr)
        state = (lstm, fc, params, opt)
    lstm, fc, params, opt = state
    y, lab = torch.as_tensor(np.asarray(rx)).double(), torch.as_tensor(np.asarray(tx)).long()
    losses = []
    for i in range(n):
        w = 0 if word_of_iter is None else int(word_of_iter[i])
        logits = fc(lstm(L.sliding_windows(y[w:w + 1]))[0]).reshape(-1, 2)
        if idx is None:
            loss = torch.nn.functional.cross_entropy(logits, lab[w])
        else:
            sel = torch.as_tensor(np.asarray(idx[i])).long()
            loss = torch.nn.functional.cross_entropy(logits[sel], lab[w][sel])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return [p.detach().numpy().copy() for p in params], np.array(losses), state


def param_bound(ref):
    return 2e-5 + 1e-3 * np.abs(ref)


def outside(got, ref):
    """Number of parameters outside |d| <= 2e-5 + 1e-3 |w| and the largest deviation."""
    n, worst = 0, 0.0
    for a, b in zip(got, ref):
        d = np.abs(np.asarray(a, np.float64) - b)
        n += int((d > param_bound(b)).sum())
        worst = max(worst, float(d.max()))
    return n, worst


def moved_fraction(start, ref):
    """Fraction of the parameters the referee moved by more than ten times the bound."""
    n = sum(int((np.abs(b - np.asarray(a, np.float64)) > 10 * param_bound(b)).sum()) for a, b in zip(start, ref))
    return n / N_PARAMS


def check_losses(got, ref):
    got = np.asarray(got, np.float64)
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"loss: largest relative deviation {rel.max():.3g}")
    assert np.all(np.abs(got - ref) <= 1e-6 + 2e-4 * np.abs(ref)), (got, ref)


def check_sgd_update(got, ref, start):
    for k, (a, b, s) in enumerate(zip(got, ref, start)):
        s = np.asarray(s, np.float64)
        du, dr = np.asarray(a, np.float64) - s, b - s
        err, nrm = np.linalg.norm(du - dr), np.linalg.norm(dr)
        print(f"SGD tensor {k}: |update - ref| / |ref| = {err / nrm:.3g}")
        assert err <= 1e-3 * nrm, (k, err, nrm)


def g18_codewords(g18):
    """G18 stores the message bits; the labels of a received word are its RS codeword (the CPU oracle's encoder)."""
    import oracle

    oracle.build()
    cw = np.asarray(oracle.rs_encode_bits(g18["tx"].astype(np.float32), int(g18["meta"][1]))).astype(np.int64)
    assert cw.shape == g18["rx"].shape and np.array_equal(cw[:, :g18["tx"].shape[1]], g18["tx"])
    return cw


def cases(g18):
    """name -> dict(ws, tx, rx, word_of_iter, idx, n, optimizer_type, lr, adam): the issue's table, T = 136."""
    gw, dw = g18_weights(g18), default_init_weights(3)
    tx, rx = g18_codewords(g18), g18["rx"]
    T = rx.shape[1]
    one = dict(tx=tx[3:4], rx=rx[3:4], word_of_iter=None)
    return {
        "g18_minibatch_adam25": dict(one, ws=gw, idx=draw_batches(T, 25, 32, 1), n=25, optimizer_type="Adam", lr=1e-3),
        "g18_whole_word_adam12": dict(one, ws=gw, idx=None, n=12, optimizer_type="Adam", lr=1e-3),
        "g18_joint_adam25": dict(ws=gw, tx=tx[1:26], rx=rx[1:26], word_of_iter=np.arange(25), idx=draw_batches(T, 25, 32, 2), n=25,
                                 optimizer_type="Adam", lr=1e-3),
        "g18_sgd6": dict(one, ws=gw, idx=draw_batches(T, 6, 32, 3), n=6, optimizer_type="SGD", lr=0.05),
        "init_adam25": dict(one, ws=dw, idx=draw_batches(T, 25, 32, 4), n=25, optimizer_type="Adam", lr=1e-3),
        # RMSprop divides every gradient by its own running magnitude, so a parameter whose gradient is within float32 rounding of
        # zero moves by up to +-10 lr whichever sign the rounding gives it, and at lr 1e-3 the iteration is not a contraction on this
        # network: with 32-position minibatches the float64 referee's own loss jumps above its start within 8 steps for every draw
        # tried (0.69 -> 1.2 ... 4.9) and stock float32 torch leaves the bound against it.  The case takes the whole word: no draws
        # to choose, and the gradients of all 136 positions keep the parameters away from that regime.
        "init_rmsprop8": dict(one, ws=dw, idx=None, n=8, optimizer_type="RMSprop", lr=1e-3),
        # ... and RMSprop with minibatches over 3 iterations from G18's weights, before that iteration has left its start
        "g18_rmsprop3_minibatch": dict(one, ws=gw, idx=draw_batches(T, 3, 32, 6), n=3, optimizer_type="RMSprop", lr=1e-3),
    }


CASE_NAMES = ["g18_minibatch_adam25", "g18_whole_word_adam12", "g18_joint_adam25", "g18_sgd6", "init_adam25", "init_rmsprop8",
              "g18_rmsprop3_minibatch"]
_REFEREE = {}


def referee_of(name, c):
    if name not in _REFEREE:
        _REFEREE[name] = referee(c["ws"], c["tx"], c["rx"], c["word_of_iter"], c["idx"], c["n"], c["optimizer_type"], c["lr"])[:2]
    return _REFEREE[name]


def start_case(c, device, use_kernel):
    """Issues the case through LSTMOnlineTrainer without reading anything back: (trainer, detector, losses on the device)."""
    det = detector_with(c["ws"], device)
    tr = mvn.LSTMOnlineTrainer(det, lr=c["lr"], use_kernel=use_kernel, optimizer_type=c["optimizer_type"])
    tx, rx = torch.from_numpy(c["tx"].astype(np.float32)).to(device), torch.from_numpy(c["rx"]).to(device)
    if c["word_of_iter"] is None:
        loss = tr.online_training(tx, rx, iterations=c["n"], batch_idx=c["idx"], full_word=c["idx"] is None, return_loss=True)
    else:
        loss = tr.train_words(tx, rx, batch_idx=c["idx"], full_word=c["idx"] is None, return_loss=True)
    return tr, det, loss


def run_case(c, device, use_kernel):
    """The case through LSTMOnlineTrainer: (final weights, losses, trainer, detector)."""
    tr, det, loss = start_case(c, device, use_kernel)
    return [p.detach().cpu().numpy() for p in tr.params], loss.cpu().numpy(), tr, det


def check_case(name, c, got, losses):
    ref, ref_losses = referee_of(name, c)
    n_out, worst = outside(got, ref)
    moved = moved_fraction(c["ws"], ref)
    print(f"{name}: {n_out} of {N_PARAMS} parameters outside the bound, largest deviation {worst:.3g}, moved > 10 x bound: {moved:.3f}")
    assert n_out == 0
    check_losses(losses, ref_losses)
    if c["optimizer_type"] == "Adam":
        assert moved > 0.9
    if c["optimizer_type"] == "SGD":
        check_sgd_update(got, ref, c["ws"])


def digest_of(ws):
    """G19's digest of ten parameter arrays: the four small tensors whole; of the six big ones 4096 entries at fixed seeded
    positions and the L2 norm."""
    out = {}
    for k, w in enumerate(ws):
        w = np.asarray(w, np.float64).reshape(-1)
        if w.size <= 4096:
            out[f"p{k}"] = w
        else:
            pos = np.random.RandomState(1900 + k).choice(w.size, 4096, replace=False)
            out[f"p{k}"] = w[pos]
            out[f"n{k}"] = np.array(np.linalg.norm(w))
    return out


def check_digest(ws, g, prefix):
    d = digest_of(ws)
    for key, v in d.items():
        ref = g[prefix + key]
        if key.startswith("n"):
            assert abs(float(v) - float(ref)) <= 1e-3 * float(ref), key
        else:
            assert np.all(np.abs(v - ref) <= param_bound(ref)), key


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lstm")


def test_symbols_bound_and_validation():
    lib = mvn._lib.load()
    for name in ("mvn_lstm_train_workspace_bytes", "mvn_lstm_train_lds_bytes", "mvn_lstm_train_f32", "mvn_lstm_train_kernel_name"):
        assert name in mvn._lib.SIGNATURES and hasattr(lib, name)
    assert lib.mvn_version() == 6
    ws = lib.mvn_lstm_train_workspace_bytes(136)
    assert ws == 384 + (2 * 136 * 256 + 4 * 1024) * 4
    assert lib.mvn_lstm_train_workspace_bytes(0) == 0 and lib.mvn_lstm_train_workspace_bytes(257) == 0
    assert lib.mvn_lstm_train_workspace_bytes(256) > ws
    fake = ctypes.c_void_p(4096)  # never dereferenced: every check below happens before a device call

    def call(T=136, y_ld=136, bits_ld=136, n_words=1, M=32, n_iter=5, ptr=fake, idx=fake, wsp=fake, wsb=ws, step0=0):
        return lib.mvn_lstm_train_f32(ptr, y_ld, ptr, bits_ld, n_words, None, idx, M, n_iter, *([ptr] * 10), ptr, ptr, step0, 1e-3,
                                      0.9, 0.999, 1e-8, None, wsp, wsb, None, T, None)

    assert call(T=0) == -1
    assert call(T=257, y_ld=300, bits_ld=300) == -1  # above MVN_LSTM_TRAIN_MAX_T
    assert call(y_ld=135) == -1 and call(bits_ld=135) == -1
    assert call(n_iter=-1) == -1
    assert call(M=-1) == -1 and call(M=137) == -1
    assert call(n_words=0) == -1
    assert call(T=0, ptr=None) == -1  # shapes before pointers
    assert call(n_iter=0, ptr=None, wsp=None) == 0  # a no-op
    assert call(ptr=None) == -4
    assert call(wsp=None) == -4
    assert call(idx=None) == -4 and call(idx=None, M=0, wsp=None) == -4
    assert call(wsb=ws - 4) == -5
    assert call(wsp=ctypes.c_void_p(4100)) == -5  # 16-byte alignment
    buf = ctypes.create_string_buffer(128)
    assert lib.mvn_lstm_train_kernel_name(136, 32, buf, 128) == 0 and b"lstm_train_kernel" in buf.value and b"minibatch" in buf.value
    assert lib.mvn_lstm_train_kernel_name(256, 0, buf, 128) == 0 and b"whole word" in buf.value
    assert lib.mvn_lstm_train_kernel_name(257, 0, buf, 128) == -1
    assert lib.mvn_lstm_train_kernel_name(136, 137, buf, 128) == -1
    assert lib.mvn_lstm_train_kernel_name(136, 0, None, 128) == -4


def test_kernel_in_code_object_no_scratch_lds_fits():
    """Read like tests/test_kernel_resources.py reads the code object: lstm_train_kernel is there, spills nothing, and its static
    LDS plus the dynamic LDS of the longest supported word stays within the 160 KB of a CU."""
    import __graft_entry__ as g

    so = g.build_hip()
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    bundler, readelf = os.path.join(llvm, "clang-offload-bundler"), os.path.join(llvm, "llvm-readelf")
    assert os.path.exists(bundler) and os.path.exists(readelf) and shutil.which("c++filt")
    import tempfile

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
    assert "lstm_train_kernel" in rows
    m = rows["lstm_train_kernel"]
    assert int(m.group(4)) == 0, f"{m.group(4)} bytes of scratch"
    lib = mvn._lib.load()
    dynamic = lib.mvn_lstm_train_lds_bytes(256)  # what the launcher asks for at the longest supported word
    assert dynamic > lib.mvn_lstm_train_lds_bytes(136) > 96 * 1024 and lib.mvn_lstm_train_lds_bytes(257) == 0
    print(f"lstm_train_kernel: {m.group(2)} VGPRs, static LDS {m.group(5)}, dynamic LDS at T = 256: {dynamic}")
    assert int(m.group(5)) + dynamic <= 160 * 1024


@pytest.mark.parametrize("name", CASE_NAMES)
def test_autograd_route_against_float64_referee(g18, name):
    c = cases(g18)[name]
    got, losses, tr, _ = run_case(c, "cpu", use_kernel=False)
    assert tr.step == c["n"] and not tr.kernel_route(136)
    check_case(name, c, got, losses)


def test_cpu_detector_takes_autograd_whatever_use_kernel_says(g18):
    c = cases(g18)["g18_whole_word_adam12"]
    c = dict(c, n=2)
    a = run_case(c, "cpu", use_kernel=True)
    b = run_case(c, "cpu", use_kernel=False)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def test_trainer_duck_type_and_arguments(g18):
    det = detector_with(g18_weights(g18))
    tr = mvn.LSTMOnlineTrainer(det)
    assert [tuple(p.shape) for p in tr.params] == L.PARAM_SHAPES and tr.params[0] is list(det.lstm.parameters())[0]
    assert tr.exp_avg.numel() == N_PARAMS == tr.exp_avg_sq.numel() and tr.step == 0
    assert tr.use_kernel is True and tr.optimizer_type == "Adam" and tr.train_minibatch_size == 32  # (the faster route)
    assert not mvn.LSTMOnlineTrainer(det, use_kernel=False).use_kernel
    assert tr.kernel_optimizer_args() == (0.9, 0.999, 1e-8)
    assert mvn.LSTMOnlineTrainer(det, optimizer_type="RMSprop").kernel_optimizer_args() == (-1.0, 0.99, 1e-8)
    assert mvn.LSTMOnlineTrainer(det, optimizer_type="SGD").kernel_optimizer_args()[0] == -2.0
    idx = tr.select_batches(136, 7)
    assert idx.shape == (7, 32) and int(idx.min()) >= 1 and int(idx.max()) < 136
    tr.check_status()  # silent
    tr.exp_avg += 1
    tr.step = 5
    tr.reset_state()
    assert tr.step == 0 and float(tr.exp_avg.abs().sum()) == 0
    with pytest.raises(NotImplementedError):
        mvn.LSTMOnlineTrainer(det, optimizer_type="Adagrad")
    with pytest.raises(ValueError):
        mvn.LSTMOnlineTrainer(mvn.VNETDetector(16, {"train": 8, "val": 8}))
    with pytest.raises(ValueError, match="batch_idx"):
        tr.online_training(torch.zeros(1, 136), torch.zeros(1, 136), iterations=3, batch_idx=torch.zeros(2, 32, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        tr.maml_training()


# ---------------------------------------------------------------------------------------------------------------------------
# golden G19 and the harness (helpers shared with the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
class ReplayDraws:
    """The `draws` of eval_by_word that replays recorded select_batch draws in call order."""

    def __init__(self, idx):
        self.idx, self.at = np.asarray(idx), 0

    def batches(self, count, N, T, iterations, minibatch):
        out = self.idx[self.at:self.at + iterations]
        self.at += iterations
        assert out.shape == (iterations, minibatch)
        return torch.from_numpy(out.astype(np.int32))


def g19_case(g19, g18, part):
    n = len(g19[part + "_loss"])
    return dict(ws=g18_weights(g18), tx=g19["a_tx"].astype(np.int64), rx=g19["a_rx"], word_of_iter=None,
                idx=torch.from_numpy(g19["a_idx"].astype(np.int32)) if part == "a" else None, n=n, optimizer_type="Adam", lr=1e-3)


def check_g19_part(g19, part, got, losses):
    check_digest(got, g19, part + "_")
    check_losses(losses, g19[part + "_loss"])


def g19_by_word(g19, g18, detector, trainer, device):
    """G19 (c) through mvn.eval_by_word: (ser_by_word, blocks that trained)."""
    iters, sub, nsym, snr, _ = [int(v) for v in g19["c_meta"]]
    tx = torch.from_numpy(g19["c_tx"].astype(np.float32)).to(device)
    rx = torch.from_numpy(g19["c_rx"]).to(device)
    draws = ReplayDraws(g19["c_idx"])
    trained = []
    ser = mvn.eval_by_word(detector, tx, rx, float(snr), 0.2, n_symbols=nsym, subframes_in_frame=sub, self_supervised=True,
                           online_trainer=trainer, self_supervised_iterations=iters, ser_thresh=float(g19["c_ser_thresh"]), draws=draws,
                           observer=lambda seen: trained.append(seen["count"]) if seen["stage"] == "end" and seen["trained"] else None)
    assert draws.at == len(g19["c_idx"]) or trained != list(g19["c_trained"])
    return ser, trained


def check_g19_by_word(g19, ser, trained):
    ref = g19["c_ser_by_word"]
    exempt = g19["c_min_margin"] < float(g19["c_margin_band"])
    data = np.arange(len(ref)) % int(g19["c_meta"][1]) != 0
    print(f"G19 c: {int((exempt & data).sum())} exempt data blocks of {int(data.sum())}, {len(g19['c_trained'])} blocks trained, "
          f"margin_band {float(g19['c_margin_band']):.3g}, blocks whose ser differs: {np.flatnonzero(ser != ref).tolist()}")
    assert (exempt & data).sum() <= 0.1 * data.sum() and len(g19["c_trained"]) >= 10
    assert trained == [int(b) for b in g19["c_trained"]]
    assert np.array_equal(ser[~exempt], ref[~exempt])


class CpuValLSTMDetector(L.LSTMDetector):
    """The detector with its 'val' decisions taken from the autograd logits (lstm_detector.py:55-57): lets the harness's update
    branch run where there is no GPU.  (The package's own 'val' is the kernel and raises on the CPU.)"""

    def forward(self, y, phase, snr=None, gamma=None, count=None):
        if phase != "val":
            return super().forward(y, phase)
        with torch.no_grad():
            return torch.argmax(super().forward(y, "train"), dim=2).float()


@pytest.fixture
def cpu_rs(monkeypatch, oracle):
    """The harness's Reed-Solomon calls on the CPU oracle."""
    monkeypatch.setattr(mvn.harness, "rs_decode", lambda w, nsym: torch.from_numpy(
        np.asarray(oracle.rs_decode_bits(w.detach().numpy().astype(np.float32), nsym), np.float32)))
    monkeypatch.setattr(mvn.harness, "rs_encode", lambda w, nsym: torch.from_numpy(
        np.asarray(oracle.rs_encode_bits(w.detach().numpy().astype(np.float32), nsym), np.float32)))


def _cpu_val_detector(ws):
    with torch.random.fork_rng(devices=[]):
        det = CpuValLSTMDetector()
    det.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(w, np.float32)) for k, w in zip(det.state_dict().keys(), ws)})
    return det


@pytest.mark.parametrize("part", ["a", "b"])
def test_g19_online_training_autograd_route(golden, g18, part):
    g19 = golden("g19_lstm_train")
    c = g19_case(g19, g18, part)
    got, losses, _, _ = run_case(c, "cpu", use_kernel=False)
    check_g19_part(g19, part, got, losses)


def test_g19_by_word_cpu_route(golden, g18, cpu_rs):
    g19 = golden("g19_lstm_train")
    det = _cpu_val_detector(g18_weights(g18))
    ser, trained = g19_by_word(g19, g18, det, mvn.LSTMOnlineTrainer(det, use_kernel=False), "cpu")
    check_g19_by_word(g19, ser, trained)


def test_meta_style_restores_the_saved_weights(golden, g18, cpu_rs):
    """meta_style_online_training=True: every training starts from the weights the run started with and uses the whole word
    (meta_lstm_trainer.py:55-60), so after the run the detector holds those weights trained on the LAST qualifying block alone."""
    g19 = golden("g19_lstm_train")
    ws = g18_weights(g18)
    det = _cpu_val_detector(ws)
    tr = mvn.LSTMOnlineTrainer(det, use_kernel=False)
    tx, rx = torch.from_numpy(g19["c_tx"][:4].astype(np.float32)), torch.from_numpy(g19["c_rx"][:4])
    seen = []
    mvn.eval_by_word(det, tx, rx, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, self_supervised=True, online_trainer=tr,
                     self_supervised_iterations=2, ser_thresh=1.0, meta_style_online_training=True, observer=seen.append)
    ends = [s for s in seen if s["stage"] == "end"]
    assert [s["trained"] for s in ends] == [True] * 4 and all(s["batch_idx"] is None for s in ends) and tr.step == 8
    # replay: every block's training from the starting weights, on one optimizer state that runs through
    det3 = _cpu_val_detector(ws)
    tr3 = mvn.LSTMOnlineTrainer(det3, use_kernel=False)
    for s in ends:
        L_tx, L_rx = s["buffer_tx"][-1].reshape(1, -1), s["buffer_rx"][-1].reshape(1, -1)
        with torch.no_grad():
            for p, w in zip(tr3.params, ws):
                p.copy_(torch.from_numpy(w))
        tr3.online_training(L_tx, L_rx, iterations=2, full_word=True)
    assert all(torch.equal(a, b) for a, b in zip(tr.params, tr3.params))


def test_harness_refusals(g18):
    ws = g18_weights(g18)
    det = _cpu_val_detector(ws)
    tx, rx = torch.zeros(3, 120), torch.zeros(3, 136)
    kw = dict(n_symbols=2, subframes_in_frame=25)
    with pytest.raises(ValueError, match="LSTMOnlineTrainer"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, self_supervised=True, **kw)
    vdet = mvn.VNETDetector(16, {"train": 136, "val": 136})
    with pytest.raises(ValueError, match="LSTMOnlineTrainer"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, self_supervised=True, online_trainer=mvn.OnlineTrainer(vdet, 4), **kw)
    with pytest.raises(ValueError, match="LSTM"):
        mvn.eval_by_word(det, tx, rx, 10.0, 0.2, online_meta=True, online_trainer=mvn.LSTMOnlineTrainer(det), **kw)
    with pytest.raises(ValueError, match="LSTM"):
        mvn.eval_by_word(L.MetaLSTMDetector(), tx, rx, 10.0, 0.2, self_supervised=True, online_trainer=mvn.LSTMOnlineTrainer(det), **kw)
    with pytest.raises(ValueError, match="LSTMOnlineTrainer"):
        mvn.eval_by_word(vdet, tx, rx, 10.0, 0.2, self_supervised=True, online_trainer=mvn.LSTMOnlineTrainer(det), **kw)
