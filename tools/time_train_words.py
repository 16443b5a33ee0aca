#!/usr/bin/env python3
"""Timing of joint training (the inner loop of Trainer.train(), trainer.py:470-479) at 16 and 128 states: n = 300 words of T = 136
symbols, a minibatch of M = 32 positions per step.

  words      ONE OnlineTrainer.train_words launch (online_train_words_kernel, mvn_vnet_train_words_f32)
  one_word   online_training(iterations=300) on ONE word in the same build -- the yardstick: its kernel is the parent commit's,
             instruction for instruction (profiles/train_words_isa_identity.txt), and does the same work per iteration
  launches   300 online_training(iterations=1) launches, a word each: joint training before the word axis
  autograd   train_words on stock autograd (use_kernel=False), 1 window

HIP events around each call, the kernel variants alternating within a round (words, one_word, launches, words, ...), WINDOWS rounds
after a warm-up round; per variant the median and (min .. max) over the rounds, in microseconds per step.  The draws, labels and
index tensors are made before the clock starts (train_words is given batch_idx and labels, online_training batch_idx and labels).
usage: time_train_words.py [output file]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_viterbinet_amd as mvn  # noqa: E402

dev = torch.device("cuda:0")
T, M, N, WINDOWS = 136, 32, 300, 7
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / N  # us per step


say(f"joint training, n = {N} words, T = {T}, M = {M}; us per step, median (min .. max) of {WINDOWS} rounds; {torch.cuda.get_device_name(0)}")
for L in (4, 7):
    S = 2 ** L
    torch.manual_seed(L)
    tx = torch.randint(0, 2, (N, T)).float().to(dev)
    rx = torch.randn(N, T, device=dev)
    labels = mvn.calculate_states(L, tx).reshape(N, T).to(torch.int32).contiguous()
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    tr = mvn.OnlineTrainer(det, L)
    idx = tr.select_batches(T, N).contiguous()
    variants = {
        "words": lambda: tr.train_words(tx, rx, batch_idx=idx, labels=labels),
        "one_word": lambda: tr.online_training(tx[:1], rx[:1], iterations=N, batch_idx=idx, labels=labels[0]),
        "launches": lambda: [tr.online_training(tx[i:i + 1], rx[i:i + 1], iterations=1, batch_idx=idx[i:i + 1], labels=labels[i])
                             for i in range(N)],
    }
    times = {k: [] for k in variants}
    for rnd in range(WINDOWS + 1):
        for k, fn in variants.items():
            t = timed(fn)
            if rnd:
                times[k].append(t)
    slow = mvn.OnlineTrainer(mvn.VNETDetector(S, {"train": T, "val": T}).to(dev), L, use_kernel=False)
    slow.train_words(tx[:10], rx[:10], batch_idx=idx[:10])
    torch.cuda.synchronize()
    times["autograd"] = [timed(lambda: slow.train_words(tx, rx, batch_idx=idx))]
    for k, v in times.items():
        say(f"S {S:4d} {k:9s} {statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})")
    w, o = statistics.median(times["words"]), times["one_word"]
    inside = min(o) <= w <= max(o)
    say(f"S {S:4d} words / one_word = {w / statistics.median(o):.4f}; the yardstick's own spread is {min(o) / statistics.median(o):.4f} .. "
        f"{max(o) / statistics.median(o):.4f} of its median: train_words is {'inside' if inside else 'OUTSIDE'} it")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
