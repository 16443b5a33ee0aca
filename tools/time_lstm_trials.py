"""The LSTM trial axis: R trials in ONE call (mvn_lstm_train_trials_f32, mvn_lstm_maml_train_trials_f32, mvn_lstm_decode_trials_f32,
trials.eval_by_word_batched with an LSTMTrialBank) against the same R trials through the single-trial entry points one after the
other, on the same GPU in the same process.  HIP events, warm, median of 5 with the spread (min .. max) beside it.
  * train:   200 minibatch iterations (M = 32) at T = 136 per trial, R = 1, 2, 4, 8
  * maml:    20 first-order meta steps at T = 136 per trial, R = 1, 2, 4, 8
  * decode:  detection of R x 1 x 136, R = 1, 2, 4, 8
  * by_word: a G19-style stretch (12 blocks, every block buffered and trained for 8 minibatch iterations) for R = 4 trials batched
             against four sequential harness.eval_by_word runs
Every measurement runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs out of
time ends the run, and nothing more is started on the GPU.
usage: time_lstm_trials.py [--out FILE] [--iters N] [--steps N] [--limit SECONDS]"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


T, M = 136, 32
ITERS, STEPS, LIMIT = arg("--iters", 200), arg("--steps", 20), arg("--limit", 240)
RS = (1, 2, 4, 8)
MEASUREMENTS = [f"{kind}:{R}" for kind in ("train", "maml", "decode") for R in RS] + ["by_word:4"]


def measure(what):
    """One measurement in this process: prints `RESULT <trials call: median min max> <single-trial calls: median min max>` in ms."""
    import torch

    import meta_viterbinet_amd as mvn
    from meta_viterbinet_amd import lstm as L

    kind, R = what.split(":")[0], int(what.split(":")[1])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    w0 = [[p.detach().clone() for p in L.LSTMDetector().to(dev)._params()] for _ in range(R)]

    def timed(fn, reps=5):
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
        return statistics.median(ts), min(ts), max(ts)

    def trainers():
        out = []
        for w in w0:
            det = L.LSTMDetector().to(dev)
            with torch.no_grad():
                for p, v in zip(det._params(), w):
                    p.copy_(v)
            out.append(mvn.LSTMMetaTrainer(det))
        return out

    gen = torch.Generator().manual_seed(1)
    bank = mvn.LSTMTrialBank(w0, dev, train_minibatch_size=M)
    everyone = list(range(R))
    if kind == "train":
        bits = torch.randint(0, 2, (R, 1, T), generator=gen).float()
        rx = ((1 - 2 * bits) + 0.5 * torch.randn(R, 1, T, generator=gen)).to(dev)
        bits_i = bits.to(dev).to(torch.int32)
        idx = torch.multinomial(torch.arange(T, dtype=torch.float32).expand(R * ITERS, T), M, generator=gen).to(torch.int32).reshape(R, ITERS, M).to(dev)
        trs = trainers()
        batched = timed(lambda: bank.train_trials(everyone, [rx[r].data_ptr() for r in everyone], [bits_i[r].data_ptr() for r in everyone],
                                                  [1] * R, [ITERS] * R, T, M, [idx[r].data_ptr() for r in everyone]))
        bank.check_status()
        bits_f = bits.to(dev)
        single = timed(lambda: [trs[r].online_training(bits_f[r], rx[r], iterations=ITERS, batch_idx=idx[r]) for r in everyone])
        for tr in trs:
            tr.check_status()
    elif kind == "maml":
        n = STEPS
        bits = torch.randint(0, 2, (R, n + 1, T), generator=gen).float()
        rx = ((1 - 2 * bits) + 0.5 * torch.randn(R, n + 1, T, generator=gen)).to(dev)
        bits_i = bits.to(dev).to(torch.int32)
        sup, qry = torch.arange(n, dtype=torch.int32, device=dev), torch.arange(1, n + 1, dtype=torch.int32, device=dev)
        trs = trainers()
        batched = timed(lambda: bank.maml_trials(everyone, [rx[r].data_ptr() for r in everyone], [bits_i[r].data_ptr() for r in everyone],
                                                 [n + 1] * R, [sup.data_ptr()] * R, [qry.data_ptr()] * R, [n] * R, T, 0.1))
        bank.check_status()
        bits_f = bits.to(dev)
        single = timed(lambda: [trs[r].maml_training(rx[r], bits_f[r], sup.reshape(n, 1), qry, 0.1, MAML=False) for r in everyone])
        for tr in trs:
            tr.check_status()
    elif kind == "decode":
        y = torch.randn(R, 1, T, generator=gen).to(dev)
        batched = timed(lambda: mvn.lstm_decode_trials(y, bank))
        single = timed(lambda: [L.lstm_decode(y[r], bank.weights(r)) for r in everyone])
    else:
        blocks = 12
        tx = torch.stack([mvn.synthetic_words(blocks, 120, 4, snr=10.0, gamma=0.2, device=dev, seed=3450002 + r)[0] for r in everyone])
        y = torch.stack([mvn.synthetic_words(blocks, T, 4, snr=10.0, gamma=0.2, device=dev, seed=3450102 + r)[1] for r in everyone])
        kw = dict(n_symbols=2, subframes_in_frame=25, self_supervised=True, self_supervised_iterations=8, ser_thresh=1.0)

        def run_batched():
            b = mvn.LSTMTrialBank(w0, dev, train_minibatch_size=M)
            mvn.eval_by_word_batched(b, tx, y, draws=[mvn.TrialDraws(5 + r, dev) for r in everyone], **kw)

        def run_single():
            for r, tr in enumerate(trainers()):
                mvn.eval_by_word(tr.detector, tx[r], y[r], 10.0, 0.2, online_trainer=tr, draws=mvn.TrialDraws(5 + r, dev), **kw)

        batched, single = timed(run_batched), timed(run_single)
    print("RESULT " + " ".join(f"{v:.6f}" for v in batched + single), flush=True)


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
        res[what] = [float(v) for v in got[-1].split()[1:]]
    import meta_viterbinet_amd as mvn

    say(f"LSTM trial axis, T = {T}: R trials in one call against R single-trial calls back to back; warm, median of 5 (min .. max), ms")
    say(f"trials per launch P = {mvn._lib.load().mvn_lstm_trials_per_launch()}")
    titles = {"train": f"training, {ITERS} minibatch iterations (M = {M}) per trial", "maml": f"meta-learning, {STEPS} first-order steps per trial",
              "decode": "detection of R x 1 words", "by_word": "by word: 12 blocks, each trained for 8 minibatch iterations"}
    for kind in ("train", "maml", "decode", "by_word"):
        rows = [(int(k.split(":")[1]), v) for k, v in res.items() if k.startswith(kind + ":")]
        if not rows:
            continue
        say(titles[kind])
        say(f"{'R':>4s} {'one call':>30s} {'R single-trial calls':>30s} {'single / one':>13s}")
        for R, (bm, blo, bhi, sm, slo, shi) in rows:
            say(f"{R:4d} {bm:12.3f} ({blo:.3f} .. {bhi:.3f}) {sm:12.3f} ({slo:.3f} .. {shi:.3f}) {sm / bm:13.2f}")
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
