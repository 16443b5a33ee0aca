"""CPU-only: the LSTM detectors (meta-viterbinet_amd/lstm.py) against golden G18 (tests/golden/make_golden_lstm.py), the C ABI's
argument checks without a device, and the C twin of the kernel (tests/native/lstm_twin.c) against a float64 nn.LSTM."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g18_weights(g):
    """The ten G18 parameters as f32 arrays (int8 multiples of a power-of-two step per tensor)."""
    return [g[f"w{i}"].astype(np.float32) * np.float32(2.0 ** int(g["w_exp"][i])) for i in range(10)]


def random_weights(seed, scale=1.0):
    """The distribution of nn.LSTM / nn.Linear's default init (every parameter ~ U(-1/16, 1/16), 1/sqrt(256)) from a seeded
    numpy stream (the global torch generators are left alone), times `scale`."""
    rng = np.random.RandomState(seed)
    return [(rng.uniform(-1 / 16, 1 / 16, s) * scale).astype(np.float32) for s in L.PARAM_SHAPES]


_TWIN = {}


def twin_lib(tmpdir):
    """gcc build of tests/native/lstm_twin.c against the CPU oracle's expf (test infrastructure)."""
    if "lib" not in _TWIN:
        import oracle

        so = oracle.build()
        out = os.path.join(str(tmpdir), "liblstm_twin.so")
        subprocess.run(["gcc", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        os.path.join(ROOT, "tests", "native", "lstm_twin.c"), "-o", out, "-L", os.path.dirname(so), "-lmvn_oracle",
                        "-Wl,-rpath," + os.path.dirname(so), "-lm"], check=True)
        lib = ctypes.CDLL(out)
        lib.lstm_twin.restype = ctypes.c_int
        lib.lstm_twin.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                  ctypes.c_void_p, ctypes.c_void_p]
        _TWIN["lib"] = lib
    return _TWIN["lib"]


def twin(tmpdir, y, weights, rows=None):
    """(logits [n, T, 2], decisions [n, T]) of the C twin for rows `rows` of y [B, T] (all rows when None)."""
    y = np.ascontiguousarray(y, np.float32)
    ws = [np.ascontiguousarray(w, np.float32) for w in weights]
    ptrs = (ctypes.c_void_p * 10)(*[w.ctypes.data for w in ws])
    r = None if rows is None else np.ascontiguousarray(rows, np.int64)
    n, T = (y.shape[0] if r is None else len(r)), y.shape[1]
    logits = np.empty((n, T, 2), np.float32)
    dec = np.empty((n, T), np.float32)
    twin_lib(tmpdir).lstm_twin(y.ctypes.data, T, ptrs, None if r is None else r.ctypes.data, n, T, logits.ctypes.data, dec.ctypes.data)
    return logits, dec


def _loaded(g):
    with torch.random.fork_rng(devices=[]):
        det = L.LSTMDetector().cpu()
    sd = {k: torch.from_numpy(w) for k, w in zip(det.state_dict().keys(), g18_weights(g))}
    det.load_state_dict(sd)
    return det


def test_symbols_bound_and_validation():
    lib = mvn._lib.load()
    for name in ("mvn_lstm_workspace_bytes", "mvn_lstm_decode_f32", "mvn_lstm_decode_kernel_name"):
        assert name in mvn._lib.SIGNATURES and hasattr(lib, name)
    assert lib.mvn_version() == 6
    ws = lib.mvn_lstm_workspace_bytes(300, 136)
    assert ws == (4 * 1024 + 3 * 1024 * 256 + 2 * 1024) * 4 and lib.mvn_lstm_workspace_bytes(0, 136) == 0
    fake = ctypes.c_void_p(4096)  # never dereferenced: every check below happens before a device call
    args = lambda y_ld, dec_ld, B, T, ptr=fake, wsp=fake, wsb=ws: (ptr, y_ld, *([ptr] * 10), ptr, dec_ld, None, wsp, wsb, B, T, None)  # noqa: E731
    call = lambda *a, **k: lib.mvn_lstm_decode_f32(*args(*a, **k))  # noqa: E731
    assert call(8, 8, 4, 0) == -1  # T < 1
    assert call(7, 8, 4, 8) == -1  # y_ld < T
    assert call(8, 7, 4, 8) == -1  # dec_ld < T
    assert call(8, 8, -1, 8) == -1
    assert call(8, 8, 0, 8, ptr=None, wsp=None) == 0  # B = 0: a no-op
    assert call(8, 8, 4, 8, ptr=None) == -4
    assert call(8, 8, 4, 8, wsp=None) == -4
    assert call(8, 8, 4, 8, wsb=ws - 4) == -5
    assert call(8, 8, 4, 8, wsp=ctypes.c_void_p(4100)) == -5  # 16-byte alignment
    buf = ctypes.create_string_buffer(128)
    for B in (1, 300, 8192):
        assert lib.mvn_lstm_decode_kernel_name(B, 136, buf, 128) == 0
        assert b"lstm_decode_kernel<1>" in buf.value and buf.value.endswith(b"x %d" % ((B + 15) // 16))
    assert lib.mvn_lstm_decode_kernel_name(-1, 136, buf, 128) == -1


def test_state_dict_matches_reference(golden):
    g = golden("g18_lstm")
    sd = L.LSTMDetector().state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for v, s in zip(sd.values(), g["shapes"]):
        assert list(v.shape) == [int(d) for d in s if d]
    assert (L.INPUT_SIZE, L.HIDDEN_SIZE, L.NUM_LAYERS, L.N_CLASSES, L.START_VALUE_PADDING) == (4, 256, 2, 2, -100)


def test_train_logits_match_reference(golden):
    g = golden("g18_lstm")
    rx, ref = torch.from_numpy(g["rx"]), g["logits"]
    det = _loaded(g)
    with torch.no_grad():
        got = det(rx, "train").numpy()
        got_meta = L.MetaLSTMDetector()(rx, "train", [torch.from_numpy(w) for w in g18_weights(g)]).numpy()
    for x in (got, got_meta):
        assert x.shape == ref.shape
        assert np.all(np.abs(x - ref) <= 1e-5 * (1 + np.abs(ref)))


def test_sliding_windows_match_reference_padding():
    y = torch.arange(1.0, 6.0).reshape(1, 5)
    x = L.sliding_windows(y)[0]
    assert x[0].tolist() == [-100, -100, -100, 1] and x[2].tolist() == [-100, 1, 2, 3] and x[4].tolist() == [2, 3, 4, 5]


def test_meta_train_double_backward():
    var = [torch.from_numpy(w).requires_grad_(True) for w in random_weights(3)]
    y = torch.randn(2, 6)
    out = L.MetaLSTMDetector()(y, "train", var)
    loss = torch.nn.functional.cross_entropy(out.reshape(-1, 2), torch.randint(0, 2, (12,)))
    grads = torch.autograd.grad(loss, var, create_graph=True)
    second = torch.autograd.grad(sum((gr * gr).sum() for gr in grads), var[1])[0]
    assert torch.isfinite(second).all() and second.abs().sum() > 0


def test_val_on_cpu_raises():
    with pytest.raises(mvn._lib.MvnError):
        L.LSTMDetector().cpu()(torch.zeros(2, 8), "val")
    with pytest.raises(mvn._lib.MvnError):
        L.MetaLSTMDetector()(torch.zeros(2, 8), "val", [torch.from_numpy(w) for w in random_weights(0)])


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_twin_matches_float64_lstm(tmp_path_factory, scale):
    w = random_weights(11, scale)
    y = torch.randn(3, 9, generator=torch.Generator().manual_seed(5)) * 1.5
    logits, dec = twin(tmp_path_factory.mktemp("twin"), y.numpy(), w)
    lstm, fc = torch.nn.LSTM(4, 256, 2, batch_first=True).double(), torch.nn.Linear(256, 2).double()
    with torch.no_grad():
        for p, a in zip(list(lstm.parameters()) + list(fc.parameters()), w):
            p.copy_(torch.from_numpy(a).double())
        ref = fc(lstm(L.sliding_windows(y.double()))[0]).numpy()
    assert np.all(np.abs(logits - ref) <= 1e-5 * (1 + np.abs(ref)))
    margin = np.abs(ref[..., 1] - ref[..., 0])
    assert np.array_equal(dec[margin > 1e-4], np.argmax(ref, axis=2).astype(np.float32)[margin > 1e-4])
