"""GPU: the LSTM detectors' 'val' kernel (mvn_lstm_decode_f32) bit for bit against the C twin (tests/native/lstm_twin.c), to
rounding against the reference (golden G18), invariant in the batch, and inside the evaluation harness."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L
from test_lstm_host import g18_weights, random_weights, twin

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _on(ws):
    return [torch.from_numpy(np.ascontiguousarray(w)).to(DEV) for w in ws]


def _det(ws):
    with torch.random.fork_rng(devices=[]):  # (the CPU generator's state stays what the tests after this file expect)
        det = L.LSTMDetector().to(DEV)
    det.load_state_dict({k: t for k, t in zip(det.state_dict().keys(), _on(ws))})
    return det


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_lstm")


def test_golden_band_rule_and_meta(g18):
    ws = g18_weights(g18)
    rx = torch.from_numpy(g18["rx"]).to(DEV)
    dec, logits = L.lstm_decode(rx, _on(ws), return_logits=True)
    ref = g18["logits"]
    assert np.all(np.abs(logits.cpu().numpy() - ref) <= 1e-4 * (1 + np.abs(ref)))
    margin = np.abs(ref[..., 1] - ref[..., 0])
    d, r = dec.cpu().numpy(), g18["dec"].astype(np.float32)
    assert np.array_equal(d[margin > 1e-4], r[margin > 1e-4])
    flips = int((d != r).sum())
    print(f"G18: {flips} in-band decision flips of {d.size}")
    det = _det(ws)
    assert torch.equal(det(rx, "val"), dec)
    assert torch.equal(L.MetaLSTMDetector()(rx, "val", _on(ws)), dec)


def test_golden_single_eval_at_point_ser(g18):
    det = _det(g18_weights(g18))
    tx = torch.from_numpy(g18["tx"].astype(np.float32)).to(DEV)
    rx = torch.from_numpy(g18["rx"]).to(DEV)
    rows = torch.from_numpy(g18["data_indices"]).to(DEV)
    ser, _, c = mvn.single_eval_at_point(det, tx, rx, 10.0, 0.2, rows=rows, n_symbols=2)
    bits = int(c[1])
    assert bits == len(g18["data_indices"]) * tx.shape[1]
    assert int(c[0]) == round(float(g18["ser"]) * bits)  # the reference's ser is a float32 mean: compare the error count
    assert ser == pytest.approx(float(g18["ser"]), rel=1e-6)


@pytest.mark.parametrize("wname", ["g18", "init", "init4x"])
def test_twin_bitwise(g18, tmp_path_factory, wname):
    ws = g18_weights(g18) if wname == "g18" else random_weights(7, 4.0 if wname == "init4x" else 1.0)
    wd = _on(ws)
    tmp = tmp_path_factory.mktemp("twin")
    gen = torch.Generator().manual_seed(99)
    for T in (1, 2, 3, 4, 136):
        for B in (1, 5, 16, 17, 33, 300):
            y = torch.randn(B, T, generator=gen) * 1.3
            dec, logits = L.lstm_decode(y.to(DEV), wd, return_logits=True)
            rows = sorted({0, B - 1, B // 2, min(B - 1, 16)})
            tl, td = twin(tmp, y.numpy(), ws, rows)
            assert _same(logits.cpu().numpy()[rows], tl), (wname, B, T)
            assert _same(dec.cpu().numpy()[rows], td), (wname, B, T)
    y = torch.randn(3, 1000, generator=gen)
    dec, logits = L.lstm_decode(y.to(DEV), wd, return_logits=True)
    tl, td = twin(tmp, y.numpy(), ws)
    assert _same(logits.cpu().numpy(), tl) and _same(dec.cpu().numpy(), td)


def test_strided_rows_and_odd_inputs(g18, tmp_path_factory):
    ws = g18_weights(g18)
    tmp = tmp_path_factory.mktemp("twin")
    base = torch.randn(19, 150, generator=torch.Generator().manual_seed(3))
    base[2, 5], base[4, 0], base[6, 40], base[6, 41] = float("nan"), float("inf"), float("-inf"), float("inf")
    y = base.to(DEV)[:, :136]  # row stride 150
    assert y.stride(0) == 150
    dec, logits = L.lstm_decode(y, _on(ws), return_logits=True)
    tl, td = twin(tmp, base[:, :136].numpy(), ws)
    assert _same(logits.cpu().numpy(), tl)
    assert np.array_equal(dec.cpu().numpy(), td)
    assert np.array_equal(dec.cpu().numpy(), torch.argmax(torch.from_numpy(tl), dim=2).float().numpy())


def test_batch_invariance_8192x1000(g18):
    wd = _on(g18_weights(g18))
    y = torch.randn(8192, 1000, generator=torch.Generator().manual_seed(8), device="cpu").to(DEV)
    dec, logits = L.lstm_decode(y, wd, return_logits=True)
    for r in (0, 4097, 8191):
        d1, l1 = L.lstm_decode(y[r:r + 1], wd, return_logits=True)
        assert torch.equal(d1[0], dec[r]) and np.array_equal(l1[0].cpu().numpy(), logits[r].cpu().numpy(), equal_nan=True)
    d2 = L.lstm_decode(y[4000:4021].clone(), wd)
    assert torch.equal(d2, dec[4000:4021])


def test_harness_accepts_the_detector(g18):
    det = _det(g18_weights(g18))
    tx = torch.from_numpy(g18["tx"].astype(np.float32)).to(DEV)
    rx = torch.from_numpy(g18["rx"]).to(DEV)
    N = 25
    ref = []
    dec = det(rx[:N], "val")
    msg = mvn.rs_decode(dec, 2)
    for k in range(N):
        errors = int((msg[k] != tx[k]).sum().item())  # decisions + RS + counting, then the reference's ser formula
        ref.append(0.0 if k % 25 == 0 else float(mvn.metrics.ser_from_errors(np.array([errors]), tx.shape[1])[0]))
    for batched in (True, False):
        got = mvn.eval_by_word(det, tx[:N], rx[:N], 10.0, 0.2, n_symbols=2, subframes_in_frame=25)
        assert np.array_equal(got, ref)
        out = mvn.detect_by_word(det, rx[:N], 10.0, 0.2, batched=batched)
        assert torch.equal(out, dec)
    c = mvn.eval_counters(det, tx, rx, 10.0, 0.2, n_symbols=2)
    assert int(c[1]) == tx.numel()
    for kw in ({"self_supervised": True}, {"online_meta": True}):
        with pytest.raises(ValueError, match="LSTM"):
            mvn.eval_by_word(det, tx[:N], rx[:N], 10.0, 0.2, n_symbols=2, subframes_in_frame=25, **kw)
