"""The dealt ViterbiNet kernel's ring-of-one form (vnet16_dealt_ring1_kernel: every wave sweeps its own range of the launch's
32-symbol units, the block loop inside, all units but a block's last whole at compile time) against the one-wave-per-block kernel
(MVN_DEALT=0) bit for bit, and a fixed sample of 64 rows against the CPU oracle.

Rings of one need at least 8 blocks per workgroup of the launch (3 workgroups per CU), so the blocks are SHORT instead of few:
    T = 32   one unit per block: every unit is a block's last, no inner loop runs
    T = 33   the last unit has one live symbol and runs as one tile
    T = 48   the last unit ends exactly at a tile edge
    T = 64   no partial unit
    T = 100  with 8 x groups + 1 blocks: the ranges do not divide, most waves have a head and a tail run
    T = 72   just above the ring-of-one threshold, and at 10 000 blocks
Each shape also runs the counting path (with and without a row mask, K < T), the final metrics, and weights that make the
strict (torch.min's NaN rule) sweep run."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn

pytestmark = pytest.mark.gpu

S = 16
# (T, blocks as a function of the launch's workgroups)
CASES = {
    "T32": (32, lambda g: 8 * g),
    "T33": (33, lambda g: 8 * g),
    "T48": (48, lambda g: 8 * g),
    "T64": (64, lambda g: 8 * g),
    "T100_ragged": (100, lambda g: 8 * g + 1),
    "T72_threshold": (72, lambda g: 8 * g + 3),
    "T72_10000": (72, lambda g: 10000),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def groups(dev):
    n_cu = ctypes.c_int()
    name = ctypes.create_string_buffer(64)
    assert mvn._lib.load().mvn_device_info(ctypes.byref(n_cu), None, name, 64) == 0, f"not a gfx950 device: {name.value!r}"
    return 3 * n_cu.value


def _np(t):
    return t.detach().cpu().numpy()


def _rand_weights(rng):
    return [rng.uniform(-1, 1, (100, 1)).astype(np.float32), rng.uniform(-1, 1, 100).astype(np.float32),
            rng.uniform(-0.1, 0.1, (50, 100)).astype(np.float32), rng.uniform(-0.1, 0.1, 50).astype(np.float32),
            rng.uniform(-0.14, 0.14, (S, 50)).astype(np.float32), rng.uniform(-0.14, 0.14, S).astype(np.float32)]


def _decode(dev, yt, wt, B, T, tx=None, K=0, mask=None):
    """mvn_vnet_decode_f32 (decisions, final metrics) or mvn_vnet_decode_count_f32 (decisions, counters) with the workspace the
    library asks for; the status word of a dealt launch must stay 0 (no hand-off abandoned)."""
    lib, st = mvn._lib.load(), mvn._lib.current_stream(dev)
    nb = int(lib.mvn_vnet_workspace_bytes(B, T, S))
    ws = torch.full((max(nb, 4),), 0x5A, dtype=torch.uint8, device=dev)  # (stale contents: the launch clears what it uses)
    dec = torch.full((B, T), 7.0, device=dev)
    wp = [mvn._lib.ptr(t) for t in wt]
    if tx is None:
        fm = torch.empty(B, S, device=dev)
        assert lib.mvn_vnet_decode_f32(mvn._lib.ptr(yt), yt.stride(0), *wp, mvn._lib.ptr(dec), T, None, mvn._lib.ptr(fm), mvn._lib.ptr(ws), nb,
                                       B, T, S, st) == 0
        out = fm
    else:
        out = torch.zeros(4, dtype=torch.int64, device=dev)
        assert lib.mvn_vnet_decode_count_f32(mvn._lib.ptr(yt), yt.stride(0), *wp, mvn._lib.ptr(tx), tx.stride(0), K, mvn._lib.ptr(mask),
                                             mvn._lib.ptr(out), mvn._lib.ptr(dec), T, mvn._lib.ptr(ws), nb, B, T, S, st) == 0
    torch.cuda.synchronize()
    if nb:
        assert int(ws[:4].view(torch.int32).item()) == 0, "a hand-off between rings was abandoned"
    return dec, out


_shapes = {}


def _shape(case, dev, groups, monkeypatch):
    """Inputs of a case and what the one-wave-per-block kernel (MVN_DEALT=0) makes of them, computed once per module; skips the
    case where this device's launch would not run rings of one."""
    if case not in _shapes:
        T, blocks = CASES[case]
        B = blocks(groups)
        lib, name = mvn._lib.load(), ctypes.create_string_buffer(96)
        assert lib.mvn_vnet_decode_kernel_name(B, T, S, 0, name, 96) == 0
        if name.value != b"vnet16_dealt_kernel<false> rings of 1":
            _shapes[case] = f"{B} blocks x {T} run {name.value.decode()!r} on this device, not the dealt kernel's rings of one"
        else:
            rng = np.random.RandomState(1000 + T + B % 977)
            w = _rand_weights(rng)
            w_nan = [a.copy() for a in w]
            w_nan[4][3, 11] = np.nan  # one NaN weight of the last layer: partially-NaN branch costs, the strict sweep
            y = rng.normal(0, 1.3, (B, T + 3)).astype(np.float32)  # (row stride > T)
            yt = torch.tensor(y, device=dev)
            wt, wt_nan = ([torch.tensor(a, device=dev) for a in ws_] for ws_ in (w, w_nan))
            monkeypatch.setenv("MVN_DEALT", "0")
            assert lib.mvn_vnet_decode_kernel_name(B, T, S, 0, name, 96) == 0 and name.value.startswith(b"vnet16_fusedn_kernel<false")
            plain = [_np(t) for t in _decode(dev, yt, wt, B, T)]
            plain_nan = [_np(t) for t in _decode(dev, yt, wt_nan, B, T)]
            monkeypatch.delenv("MVN_DEALT")
            rows = np.sort(np.random.RandomState(7).choice(B, 64, replace=False))
            rows[0], rows[-1] = 0, B - 1
            _shapes[case] = dict(B=B, T=T, w=w, w_nan=w_nan, y=y, yt=yt, wt=wt, wt_nan=wt_nan, plain=plain, plain_nan=plain_nan, rows=rows)
    if isinstance(_shapes[case], str):
        pytest.skip(_shapes[case])
    return _shapes[case]


@pytest.mark.parametrize("case", list(CASES))
def test_ring1_decisions_and_final_metrics(oracle, dev, groups, monkeypatch, case):
    """Decisions and final metrics equal the one-wave-per-block kernel's bit for bit; 64 rows equal the oracle's."""
    c = _shape(case, dev, groups, monkeypatch)
    dec, fm = (_np(t) for t in _decode(dev, c["yt"], c["wt"], c["B"], c["T"]))
    assert np.array_equal(dec, c["plain"][0])
    assert np.array_equal(fm, c["plain"][1])
    rdec, rfm = oracle.vnet_decode(np.ascontiguousarray(c["y"][c["rows"], :c["T"]]), c["w"], want_final=True)
    assert np.array_equal(dec[c["rows"]], rdec) and np.array_equal(fm[c["rows"]], rfm)


@pytest.mark.parametrize("masked", [False, True], ids=["all_rows", "row_mask"])
@pytest.mark.parametrize("case", list(CASES))
def test_ring1_counting(oracle, dev, groups, monkeypatch, case, masked):
    """mvn_vnet_decode_count_f32 on rings of one, K < T: the decisions are the plain kernel's and the counters are count_errors of
    them, over all rows and over the rows of a mask."""
    c = _shape(case, dev, groups, monkeypatch)
    B, T = c["B"], c["T"]
    K = max(1, T - 5)
    tx = np.random.RandomState(T + masked).randint(0, 2, (B, K)).astype(np.float32)
    rows = np.array([i for i in range(B) if i % 5 != 0], np.int64) if masked else np.arange(B, dtype=np.int64)
    mask = None
    if masked:
        mask = torch.zeros(B, dtype=torch.uint8, device=dev)
        mask[torch.tensor(rows, device=dev)] = 1
    dec, cnt = _decode(dev, c["yt"], c["wt"], B, T, tx=torch.tensor(tx, device=dev), K=K, mask=mask)
    assert np.array_equal(_np(dec), c["plain"][0])
    assert cnt.tolist() == oracle.count_errors(c["plain"][0][:, :K], tx, rows).tolist()


@pytest.mark.parametrize("case", list(CASES))
def test_ring1_strict(oracle, dev, groups, monkeypatch, case):
    """A NaN weight makes the launch strict: torch.min's NaN rule in the whole units' sweeps and in the peeled last unit."""
    c = _shape(case, dev, groups, monkeypatch)
    dec, fm = (_np(t) for t in _decode(dev, c["yt"], c["wt_nan"], c["B"], c["T"]))
    assert np.array_equal(dec, c["plain_nan"][0], equal_nan=True)
    assert np.array_equal(fm, c["plain_nan"][1], equal_nan=True)
    rdec, rfm = oracle.vnet_decode(np.ascontiguousarray(c["y"][c["rows"], :c["T"]]), c["w_nan"], want_final=True)
    assert np.array_equal(dec[c["rows"]], rdec, equal_nan=True) and np.array_equal(fm[c["rows"]], rfm, equal_nan=True)
