"""The LSTM detector's 'val' path (mvn_lstm_decode_f32: weight packing + lstm_decode_kernel) against two baselines on the same GPU
in the same run: one batched nn.LSTM call (MIOpen) + fc + argmax, and the reference's pattern of one nn.LSTM call per word
(lstm_detector.py:48-50).  HIP-event timings, best of 3 repetitions; FLOP counted at 1.582 MFLOP per symbol (791 040 MACs).
usage: time_lstm.py [--per-word-max B]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_viterbinet_amd as mvn  # noqa: E402
from meta_viterbinet_amd import lstm as L  # noqa: E402

FLOP_PER_SYMBOL = 2 * (1024 * (4 + 256) + 1024 * 512 + 2 * 256)  # 791 040 MACs
PEAK = 157.3e12
dev = torch.device("cuda:0")
torch.manual_seed(0)
det = L.LSTMDetector().to(dev)
params = det._params()


def timed(fn, reps=3, inner=1):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) / inner)
    return best


@torch.no_grad()
def batched_torch(y, chunk=None):
    if chunk:  # MIOpen rejects 8192 x 1000 in one call ("Strides must be > 0"): the batch in slices of `chunk` words
        return torch.cat([batched_torch(y[i:i + chunk]) for i in range(0, y.shape[0], chunk)])
    out, _ = det.lstm(L.sliding_windows(y))
    return torch.argmax(det.fc(out), dim=2).float()


@torch.no_grad()
def per_word_torch(y):
    x = L.sliding_windows(y)
    out = torch.empty(y.shape[0], y.shape[1], 256, device=y.device)
    for i in range(y.shape[0]):
        out[i] = det.lstm(x[i:i + 1])[0][0]
    return torch.argmax(det.fc(out), dim=2).float()


per_word_max = int(sys.argv[sys.argv.index("--per-word-max") + 1]) if "--per-word-max" in sys.argv else 300
print(f"{'shape':>12s} {'kernel ms':>10s} {'of peak':>8s} {'batched nn.LSTM ms':>19s} {'per-word nn.LSTM ms':>20s}  kernel form")
for B, T in ((8192, 1000), (300, 136), (1, 136)):
    y = torch.randn(B, T, device=dev)
    tk = timed(lambda: L.lstm_decode(y, params), inner=1 if B * T > 10 ** 6 else 5)
    assert torch.equal(L.lstm_decode(y, params), L.lstm_decode(y, params))
    chunk = 1024 if B * T > 4 * 10 ** 6 else None
    tb = timed(lambda: batched_torch(y, chunk))
    tw = timed(lambda: per_word_torch(y), reps=1) if B <= per_word_max else float("nan")
    buf = __import__("ctypes").create_string_buffer(128)
    mvn._lib.load().mvn_lstm_decode_kernel_name(B, T, buf, 128)
    frac = FLOP_PER_SYMBOL * B * T / (tk * 1e-3) / PEAK
    note = f" (nn.LSTM in slices of {chunk} words)" if chunk else ""
    print(f"{B:>6d}x{T:<5d} {tk:10.3f} {frac:8.3f} {tb:19.3f} {tw:20.3f}  {buf.value.decode()}{note}", flush=True)
