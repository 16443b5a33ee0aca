#!/usr/bin/env python3
"""One Monte-Carlo point of the 16-state ViterbiNet: the launch that generates its words inside the detector
(mvn_vnet_montecarlo_f32 / vnet16_mc_kernel: nothing but four counters written) against generate_words -> val_count, the two launches
it replaces, in the same build.  HIP events around each call, both routes warm, alternated, the median of the repetitions; the
counters of the two routes are compared first.  Also the run-to-F-frame-errors form: 16 rounds with a target that the 8th round
reaches, against 16 single calls with a host read of the counters after each (what a host loop over chunks has to do).
usage: time_vnet_montecarlo.py [repetitions]"""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_viterbinet_amd as mvn  # noqa: E402

dev = torch.device("cuda:0")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
S, L, T, SNR, GAMMA, SEED = 16, 4, 1000, 10.0, 0.2, 7


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def medians(fns, reps=REPS):
    """Median milliseconds of each of `fns`, alternated within every repetition (two warm-up passes first)."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for ts, fn in zip(times, fns):
            ts.append(event_ms(fn))
    return [(statistics.median(ts), min(ts), max(ts)) for ts in times]


det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
g7 = np.load(os.path.join(ROOT, "tests", "golden", "g7_by_word.npz"))  # the reference-trained 16-state weights
with torch.no_grad():
    for k, p in enumerate(det.net.parameters()):
        p.copy_(torch.from_numpy(g7[f"w{k}"]))
h = mvn.estimate_channel(L, GAMMA, "time_decay")
hd = torch.as_tensor(h, device=dev)
lib = mvn._lib.load()

print(f"{torch.cuda.get_device_name(0)}; {REPS} repetitions, HIP events, median (min .. max) in ms; T = {T}, {SNR} dB", flush=True)
for B in (10000, 100000):
    def two():
        tx, y = mvn.generate_words(B, T, h, SNR, L, dev, SEED)
        return det.val_count(y, tx)

    def one():
        return mvn.vnet_monte_carlo(det, B, hd, SNR, dev, SEED)

    want, got = two().tolist(), one().tolist()
    tx, y = mvn.generate_words(B, T, h, SNR, L, dev, SEED)
    buf = ctypes.create_string_buffer(96)
    lib.mvn_vnet_decode_kernel_name(B, T, S, 0, buf, 96)
    (t2, t1, td, tg) = medians([two, one, lambda: det.val_count(y, tx), lambda: mvn.generate_words(B, T, h, SNR, L, dev, SEED)])
    print(f"{B:7d} x {T}: generate_words + val_count {t2[0]:8.3f} ({t2[1]:.3f} .. {t2[2]:.3f})   "
          f"[val_count alone, {buf.value.decode()}: {td[0]:8.3f}; generate_words alone: {tg[0]:8.3f}]   "
          f"one launch (vnet16_mc_kernel) {t1[0]:8.3f} ({t1[1]:.3f} .. {t1[2]:.3f}) = {B * T / t1[0] / 1e6:6.2f} Gsym/s, "
          f"{t1[0] / t2[0]:5.3f} x the two launches, {t1[0] / td[0]:5.3f} x the detector alone   "
          f"words in device memory {8 * B * T / 1e6:7.1f} MB -> 0   counters equal {got == want}  ser {got[0] / got[1]:.5f}", flush=True)
    del tx, y

# run to F frame errors: 16 rounds of 10 000 words, the target placed so that 8 rounds run
B, ROUNDS = 10000, 16
per_round = [mvn.vnet_monte_carlo(det, B, hd, SNR, dev, SEED, first_word=r * B).tolist() for r in range(ROUNDS)]
F = sum(r[2] for r in per_round[:8])


def on_device():
    return mvn.vnet_monte_carlo(det, B, hd, SNR, dev, SEED, rounds=ROUNDS, stop_frame_errors=F)


def host_loop():
    c = torch.zeros(4, dtype=torch.int64, device=dev)
    for r in range(ROUNDS):
        mvn.vnet_monte_carlo(det, B, hd, SNR, dev, SEED, counters=c, first_word=r * B)
        if c[2].item() >= F:  # the host has to read the counters to decide whether to go on
            break
    return c


c, ran = on_device()
(tg_, th_) = medians([on_device, host_loop])
print(f"run to {F} frame errors, {ROUNDS} rounds of {B} x {T} enqueued: {int(ran.item())} rounds ran, counters equal the host loop's "
      f"{c.tolist() == host_loop().tolist()}   gated on the device, no synchronisation {tg_[0]:8.3f} ({tg_[1]:.3f} .. {tg_[2]:.3f})   "
      f"host loop with one counter read per round {th_[0]:8.3f} ({th_[1]:.3f} .. {th_[2]:.3f})", flush=True)
