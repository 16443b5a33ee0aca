"""Online meta-learning of the LSTM detector: the one-launch first-order kernel (mvn_lstm_maml_train_f32 behind
LSTMMetaTrainer) against the autograd route (use_kernel=False: MetaLSTMDetector unrolled on torch autograd + the optimizer step in
torch ops) on the same GPU in the same run.  HIP events, warm, median of 5.
  * first-order meta steps at T = 136 on the kernel and through autograd, second-order steps through autograd, per step
  * one G20-style by-word stretch (6 blocks of eval_by_word with online_meta, first order: ONE meta update of 2 x <= 3 steps at
    block 5, 4 whole-word iterations after every block), both ways
Every measurement runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out of
time ends the run, and nothing more is started on the GPU.
usage: time_lstm_meta.py [--out FILE] [--steps N] [--autograd-steps N] [--limit SECONDS]"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


T = 136
STEPS, AG_STEPS, LIMIT = arg("--steps", 20), arg("--autograd-steps", 2), arg("--limit", 240)
MEASUREMENTS = ("kernel", "autograd", "second", "by_word_kernel", "by_word_autograd")


def measure(what):
    """One measurement in this process: prints `RESULT <ms>` (the median of 5 warm runs)."""
    import torch

    import meta_viterbinet_amd as mvn
    from meta_viterbinet_amd import lstm as L

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    w0 = [p.detach().clone() for p in L.LSTMDetector().to(dev)._params()]

    def fresh(use_kernel):
        det = L.LSTMDetector().to(dev)
        with torch.no_grad():
            for p, w in zip(det._params(), w0):
                p.copy_(w)
        return det, mvn.LSTMMetaTrainer(det, use_kernel=use_kernel)

    def median_ms(fn, reps=5):
        fn()  # warm
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

    if what in ("kernel", "autograd", "second"):
        n = STEPS if what == "kernel" else AG_STEPS
        gen = torch.Generator().manual_seed(1)
        bits = torch.randint(0, 2, (n + 1, T), generator=gen).float()
        rx = ((1 - 2 * bits) + 0.5 * torch.randn(n + 1, T, generator=gen)).to(dev)
        bits = bits.to(dev)
        sup, qry = torch.arange(n).reshape(n, 1), torch.arange(1, n + 1)
        det, tr = fresh(what == "kernel")
        assert tr.meta_kernel_route(T, 1, what == "second") == (what == "kernel")
        ms = median_ms(lambda: tr.maml_training(rx, bits, sup, qry, 0.1, MAML=what == "second")) / n
        tr.check_status()
    else:
        blocks = 6
        tx, _ = mvn.synthetic_words(blocks, 120, 4, snr=10.0, gamma=0.2, device=dev, seed=3450002)
        _, y = mvn.synthetic_words(blocks, T, 4, snr=10.0, gamma=0.2, device=dev, seed=3450003)

        def run():
            torch.manual_seed(2)  # the same j_hat draws every time
            det, tr = fresh(what == "by_word_kernel")
            mvn.eval_by_word(det, tx, y, 10.0, 0.2, n_symbols=2, subframes_in_frame=25, self_supervised=True, online_trainer=tr,
                             self_supervised_iterations=4, ser_thresh=1.0, online_meta=True, MAML=False, meta_lr=0.1,
                             meta_train_iterations=2, meta_j_num=3, meta_subframes=5, meta_style_online_training=True)

        ms = median_ms(run)
    print(f"RESULT {ms:.6f}", flush=True)


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = {}
    for what in MEASUREMENTS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", what] + sys.argv[1:], capture_output=True, text=True,
                               timeout=LIMIT)
        except subprocess.TimeoutExpired:
            say(f"{what}: no result within {LIMIT} s; nothing further was started")
            break
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            say(f"{what}: exit status {r.returncode}; nothing further was started")
            sys.stderr.write(r.stderr[-2000:])
            break
        res[what] = float(got[-1].split()[1])
    say(f"LSTM online meta-learning, T = {T}, warm, median of 5 (ms)")
    if "kernel" in res:
        say(f"{'first order, kernel':>28s} {res['kernel']:10.3f} per step   ({STEPS} steps per call)")
    if "autograd" in res:
        say(f"{'first order, autograd':>28s} {res['autograd']:10.3f} per step   ({AG_STEPS} steps per call)")
    if "second" in res:
        say(f"{'second order, autograd':>28s} {res['second']:10.3f} per step   ({AG_STEPS} steps per call)")
    if "kernel" in res and "autograd" in res:
        say(f"{'autograd / kernel':>28s} {res['autograd'] / res['kernel']:10.1f}   (first order)")
    if "by_word_kernel" in res:
        say("eval_by_word, online_meta, first order: 6 blocks, one meta update (2 x <= 3 steps) at block 5, 4 whole-word iterations after "
            "every block (ms)")
        say(f"{'kernel':>28s} {res['by_word_kernel']:10.2f}")
    if "by_word_autograd" in res:
        say(f"{'autograd':>28s} {res['by_word_autograd']:10.2f}   autograd / kernel {res['by_word_autograd'] / res['by_word_kernel']:.1f}")
    out = arg("--out", "")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if len(res) == len(MEASUREMENTS) else 1


if __name__ == "__main__":
    if "--measure" in sys.argv:
        measure(sys.argv[sys.argv.index("--measure") + 1])
    else:
        sys.exit(main())
