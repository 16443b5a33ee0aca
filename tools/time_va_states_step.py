"""The classical Viterbi detector's by-word block steps at 4, 8, 32, 64 and 128 states (mvn_va_byword_step_states_f32, _path_f32,
_list_f32) against what a block cost before them, on the same build.

Per S, one data block of T = 136 symbols (nsym = 2), R = 1 word, as harness.eval_by_word issues it: the work of the block and the copy
of its error count to the host, on a host clock around the synchronising copy.
  running  one launch : mvn_va_byword_step_states_f32 (dec, enc, nerr) + nerr to the host
           separate   : detector(rx, 'val', snr, gamma), rs_decode, the error count, rs_encode + nerr to the host (eval_by_word with
                        fused_step=False)
  path     one launch : mvn_va_byword_step_states_path_f32 + nerr to the host
           separate   : detector.viterbi_path(rx, snr, gamma) (the sweep with survivors, the traceback), rs_decode, the error count,
                        rs_encode + nerr to the host
  list     one launch : mvn_va_byword_step_states_list_f32 (list_bytes = 4) + nerr to the host, against the path step's one launch
                        (there is no other route to a list decode)
The two sides of a row alternate, REPEATS windows of ITERS blocks each after a warm-up of both; median and (min .. max) of the windows,
microseconds per block.  Every S runs in a child process of its own under `timeout`, so one that hangs ends alone; after a child that
fails nothing more is started on the device.

    python tools/time_va_states_step.py [out.txt]     everything (the table of profiles/va_states_step_time.txt)
    python tools/time_va_states_step.py --step S      one state count (what the children run)
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, NSYM, LIST_BYTES, ITERS, REPEATS, CHILD_TIMEOUT_S = 136, 2, 4, 100, 7, 240
SNR, GAMMA = 7.0, 0.2


def _spread(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def _race(label, S, a, b, names):
    ts = {a: [], b: []}
    for fn in ts:  # warm
        for _ in range(20):
            fn()
    for _ in range(REPEATS):
        for fn in ts:
            t0 = time.perf_counter()
            for _ in range(ITERS):
                fn()
            ts[fn].append((time.perf_counter() - t0) / ITERS * 1e6)
    ma, mb = statistics.median(ts[a]), statistics.median(ts[b])
    print(f"{label:7s} S {S:3d}: {names[0]} {_spread(ts[a])} us, {names[1]} {_spread(ts[b])} us per block ({mb / ma:4.2f} x)", flush=True)


def _step(S):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn

    dev = torch.device("cuda:0")
    L, K = int(np.log2(S)), T - 8 * NSYM
    gen = torch.Generator(device=dev).manual_seed(S)
    det = mvn.VADetector(S, L, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    msg = torch.randint(0, 2, (1, K), generator=gen, device=dev).float()
    rx = mvn.transmit(mvn.rs_encode(msg, NSYM), mvn.estimate_channel(L, GAMMA, "time_decay"), SNR, L, torch.randn(1, T, generator=gen, device=dev))
    pri = det._priors_table(rx, GAMMA, "val", None)
    front = (mvn._lib.ptr(pri), 1)
    dec, enc = torch.empty(1, T, device=dev), torch.empty(1, T, device=dev)
    nerr = torch.empty(1, dtype=torch.int32, device=dev)
    out = {"dec": (mvn._lib.ptr(dec), T), "enc": (mvn._lib.ptr(enc), T)}
    steps = {d: mvn._lib.BywordStep("va", d, T, NSYM, LIST_BYTES if d == "list" else None, n_states=S, states_va=True)
             for d in ("running", "path", "list")}

    def one_launch(decision):
        def run():
            steps[decision](dev, mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, front, out, mvn._lib.ptr(nerr), 1, False)
            return nerr.cpu()
        return run

    def separate(detect):
        def run():
            m = mvn.rs_decode(detect(), NSYM)
            e = (m != msg).sum(dim=1)
            mvn.rs_encode(m, NSYM)
            return e.cpu()
        return run

    detect = {"running": lambda: det(rx, "val", SNR, GAMMA), "path": lambda: det.viterbi_path(rx, SNR, GAMMA)}
    for decision in ("running", "path"):
        a, b = one_launch(decision), separate(detect[decision])
        assert torch.equal(a().long(), b().long()) and torch.equal(dec, detect[decision]())
        _race(decision, S, a, b, ("one launch", "separate launches"))
    _race("list", S, one_launch("list"), one_launch("path"), ("list step", "path step"))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        _step(int(sys.argv[2]))
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for S in (4, 8, 32, 64, 128):
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", str(S)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        text = res.stdout.strip() if res.returncode == 0 else f"--step {S}: exit status {res.returncode}\n{res.stdout}{res.stderr[-2000:]}"
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        if res.returncode != 0:  # a fault, abort or time limit: nothing more is started on the device
            sys.exit(1)


if __name__ == "__main__":
    main()
