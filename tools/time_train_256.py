#!/usr/bin/env python3
"""Timing: 200 online-training iterations on one word of 136 symbols at 256 states (channel memory 8) -- online_train_kernel<256,
false> with minibatches of 32 and on the whole word, OnlineTrainer(use_kernel=False) (stock autograd + the shared optimizer state:
what every call at 256 states ran before the kernel existed) on the same word and draws, and the 128-state kernel alongside.  One
build, one process.  Every figure is the median over REPS calls after WARM discarded ones (the clocks settle), with the smallest
and the largest call beside it; a call is timed with device events around the launch (kernel routes) or the loop (autograd).

    python tools/time_train_256.py [output file]

Exit status 1 if the kernel route at 256 states is less than 10 x as fast as the autograd route measured beside it."""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_viterbinet_amd as mvn  # noqa: E402

dev = torch.device("cuda:0")
T, N, M = 136, 200, 32
WARM, REPS = 3, 10
WARM_AUTOGRAD, REPS_AUTOGRAD = 1, 3


def setup(S, use_kernel):
    L = S.bit_length() - 1
    torch.manual_seed(S)
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    tr = mvn.OnlineTrainer(det, L, use_kernel=use_kernel)
    gen = torch.Generator().manual_seed(7)
    tx = torch.randint(0, 2, (1, T), generator=gen).float().to(dev)
    rx = torch.randn(1, T, generator=gen).to(dev)
    idx = torch.stack([torch.randperm(T - 1, generator=gen)[:M] + 1 for _ in range(N)]).to(torch.int32).to(dev)
    return tr, tx, rx, idx


def timed(S, use_kernel, full_word, warm, reps):
    tr, tx, rx, idx = setup(S, use_kernel)
    ms = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        tr.online_training(tx, rx, iterations=N, batch_idx=None if full_word else idx, full_word=full_word)
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    tr.check_status()
    return statistics.median(ms), min(ms), max(ms)


def kernel_name(S, full_word):
    name = ctypes.create_string_buffer(96)
    assert mvn._lib.load().mvn_vnet_train_kernel_name(0, 0, T, 0 if full_word else M, S, 0, name, 96) == 0
    return name.value.decode()


def main():
    lines = [f"{N} online-training iterations on one word, T = {T}; per call: median [min .. max] over {REPS} calls after {WARM} discarded"
             f" ({REPS_AUTOGRAD} after {WARM_AUTOGRAD} for autograd); device {torch.cuda.get_device_name(0)}"]
    fig = {}
    for S in (256, 128):
        for full_word in (False, True):
            what = "whole word" if full_word else f"minibatch {M}"
            med, lo, hi = timed(S, True, full_word, WARM, REPS)
            fig[(S, full_word, True)] = med
            lines.append(f"  S = {S:3d} {what:12s} {kernel_name(S, full_word):38s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {med / N * 1e3:8.1f} us/iteration")
    for full_word in (False, True):
        what = "whole word" if full_word else f"minibatch {M}"
        med, lo, hi = timed(256, False, full_word, WARM_AUTOGRAD, REPS_AUTOGRAD)
        fig[(256, full_word, False)] = med
        lines.append(f"  S = 256 {what:12s} {'OnlineTrainer(use_kernel=False), autograd':38s} {med:9.3f} ms [{lo:.3f} .. {hi:.3f}]  {med / N * 1e3:8.1f} us/iteration")
    ok = True
    for full_word in (False, True):
        ratio = fig[(256, full_word, False)] / fig[(256, full_word, True)]
        ok = ok and ratio >= 10.0
        lines.append(f"  256 states, {'whole word' if full_word else f'minibatch {M}'}: the kernel is {ratio:.1f} x as fast as autograd (required: 10 x);"
                     f" {fig[(256, full_word, True)] / fig[(128, full_word, True)]:.2f} x the 128-state kernel's time")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
