"""Training of the LSTM detector: the one-launch kernel (mvn_lstm_train_f32 behind LSTMOnlineTrainer) against the autograd route
(use_kernel=False: nn.LSTM autograd + the optimizer step in torch ops -- what a user could do before the kernel existed) on the same
GPU in the same run.  HIP events, warm, median of 5.
  * 200 iterations on one word of T = 136: 32-position minibatches and the whole word
  * one 100-block eval_by_word with self_supervised=True (200 iterations after every block) through the kernel; the autograd route
    on the first few blocks (it takes seconds per block), both reported per block
usage: time_lstm_train.py [--out FILE] [--blocks N] [--autograd-blocks N] [--iterations N]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import meta_viterbinet_amd as mvn  # noqa: E402
from meta_viterbinet_amd import lstm as L  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


dev = torch.device("cuda:0")
T, ITER, BLOCKS = 136, arg("--iterations", 200), arg("--blocks", 100)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn, reps=5, warm=True):
    if warm:
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


torch.manual_seed(0)
start = L.LSTMDetector().to(dev)
w0 = [p.detach().clone() for p in start._params()]
gen = torch.Generator().manual_seed(1)
bits = torch.randint(0, 2, (1, T), generator=gen).float().to(dev)
rx = ((1 - 2 * bits.cpu()) + 0.5 * torch.randn(1, T, generator=gen)).to(dev)


def fresh(use_kernel):
    det = L.LSTMDetector().to(dev)
    with torch.no_grad():
        for p, w in zip(det._params(), w0):
            p.copy_(w)
    return det, mvn.LSTMOnlineTrainer(det, use_kernel=use_kernel)


say(f"LSTM training, T = {T}, {ITER} iterations per call, median of 5 (ms)")
say(f"{'form':>12s} {'kernel':>10s} {'per iter':>9s} {'autograd':>10s} {'per iter':>9s} {'autograd / kernel':>18s}")
for name, full in (("minibatch", False), ("whole word", True)):
    res = {}
    for use_kernel in (True, False):
        det, tr = fresh(use_kernel)
        idx = None if full else tr.select_batches(T, ITER)
        res[use_kernel] = median_ms(lambda: tr.online_training(bits, rx, iterations=ITER, batch_idx=idx, full_word=full))
        tr.check_status()
    say(f"{name:>12s} {res[True]:10.2f} {res[True] / ITER:9.4f} {res[False]:10.2f} {res[False] / ITER:9.3f} {res[False] / res[True]:18.1f}")

# one by-word evaluation with the update branch: words of a 10-dB ISI channel, every block qualifies (ser_thresh 1).  The detector
# and the trainer are built outside the timed region.  The autograd route takes seconds per block, so it is timed on the first
# AG_BLOCKS blocks only (every block costs the same: one detection, RS, 200 iterations) and reported per block beside the kernel's.
AG_BLOCKS = arg("--autograd-blocks", 4)
tx, _ = mvn.synthetic_words(BLOCKS, 120, 4, snr=10.0, gamma=0.2, device=dev, seed=3450002)
_, y = mvn.synthetic_words(BLOCKS, T, 4, snr=10.0, gamma=0.2, device=dev, seed=3450003)


def by_word_ms(use_kernel, blocks, reps=5):
    ts = []
    for rep in range(reps + 1):  # the first run warms and is not counted
        det, tr = fresh(use_kernel)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        mvn.eval_by_word(det, tx[:blocks], y[:blocks], 10.0, 0.2, n_symbols=2, subframes_in_frame=25, self_supervised=True,
                         online_trainer=tr, self_supervised_iterations=ITER, ser_thresh=1.0)
        b.record()
        b.synchronize()
        print(".", end="", flush=True)
        if rep:
            ts.append(a.elapsed_time(b))
    print()
    return statistics.median(ts)


say(f"eval_by_word, self_supervised, {ITER} iterations after every block, warm, median of 5 (ms)")
tk = by_word_ms(True, BLOCKS)
tk_few = by_word_ms(True, AG_BLOCKS)
ta_few = by_word_ms(False, AG_BLOCKS)
say(f"{'kernel':>12s} {BLOCKS:4d} blocks {tk:10.1f}  per block {tk / BLOCKS:8.2f}")
say(f"{'kernel':>12s} {AG_BLOCKS:4d} blocks {tk_few:10.1f}  per block {tk_few / AG_BLOCKS:8.2f}")
say(f"{'autograd':>12s} {AG_BLOCKS:4d} blocks {ta_few:10.1f}  per block {ta_few / AG_BLOCKS:8.2f}   (cut to {AG_BLOCKS} blocks: {BLOCKS} would take "
    f"about {ta_few / AG_BLOCKS * BLOCKS / 1000:.0f} s per run)   autograd / kernel {ta_few / tk_few:.1f}")
out = arg("--out", "")
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
