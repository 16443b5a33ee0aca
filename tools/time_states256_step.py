"""The by-word block steps at 256 states (mvn_vnet_byword_step_256_f32, _256_path_f32, mvn_va_byword_step_256_f32, _256_path_f32)
against the separate launches of the same build -- the route eval_by_word(fused_step=False) takes and every earlier version took at
256 states.

  per kernel (ViterbiNet / classical x running / path), one data block of T = 136 symbols (nsym = 2) for R = 1 / 6 / 256 words, as
  the by-word evaluation issues it: the work of the block and the copy of its error counts to the host, on a host clock around the
  synchronising copy.
    one launch : the 256-state step (dec, enc, nerr) + nerr to the host
    separate   : detector(rx, 'val') or detector.viterbi_path(rx), rs_decode, the error count, rs_encode + nerr to the host
  The two alternate, REPEATS windows of ITERS blocks each; median and (min .. max) of the windows, microseconds per block.
Every kernel runs in a child process of its own under `timeout`, so one that hangs ends alone; after a child that fails nothing more
is started on the device.

    python tools/time_states256_step.py [out.txt]            everything (the table of profiles/states256_step_time.txt)
    python tools/time_states256_step.py --step KIND DECISION  one kernel (what the children run)
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, L, T, NSYM, ITERS, REPEATS, CHILD_TIMEOUT_S = 256, 8, 136, 2, 100, 7, 300
GAMMA, SNR_DB = 0.2, 9.0
WEIGHTS = ("g23_by_word_256_states", "L8_selfsup_w0_%d")  # weights the reference's trainer produced at memory 8


def _spread(ts):
    return f"{statistics.median(ts):8.1f} ({min(ts):.1f} .. {max(ts):.1f})"


def _step(kind, decision):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn

    dev = torch.device("cuda:0")
    K = T - 8 * NSYM
    gen = torch.Generator(device=dev).manual_seed(S)
    if kind == "vnet":
        det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
        g = np.load(os.path.join(ROOT, "tests", "golden", WEIGHTS[0] + ".npz"))
        with torch.no_grad():
            for i, p in enumerate(det.parameters()):
                p.copy_(torch.tensor(g[WEIGHTS[1] % i]).reshape(p.shape))
        front = (*[mvn._lib.ptr(mvn._lib.f32c(p)) for p in det._params()], None)
        detect = (lambda y: det(y, "val")) if decision == "running" else (lambda y: det.viterbi_path(y))
    else:
        det = mvn.VADetector(S, L, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
        detect = ((lambda y: det(y, "val", SNR_DB, GAMMA)) if decision == "running" else
                  (lambda y: det.viterbi_path(y, SNR_DB, GAMMA)))
    step = mvn._lib.BywordStep(kind, decision, T, NSYM, n_states=S, states_256=True)
    for R in (1, 6, 256):
        msg = torch.randint(0, 2, (R, K), generator=gen, device=dev).float()
        rx = mvn.transmit(mvn.rs_encode(msg, NSYM), mvn.estimate_channel(L, GAMMA, "time_decay"), SNR_DB, L,
                          torch.randn(R, T, generator=gen, device=dev))
        if kind == "va":
            pri = det._priors_table(rx, GAMMA, "val", None)
            front = (mvn._lib.ptr(pri), 1)
        dec, enc = torch.empty(R, T, device=dev), torch.empty(R, T, device=dev)
        nerr = torch.empty(R, dtype=torch.int32, device=dev)
        out = {"dec": (mvn._lib.ptr(dec), T), "enc": (mvn._lib.ptr(enc), T)}

        def one_launch():
            step(dev, mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, front, out, mvn._lib.ptr(nerr), R, False)
            return nerr.cpu()

        def separate():
            d = detect(rx)
            m = mvn.rs_decode(d, NSYM)
            e = (m != msg).sum(dim=1)
            mvn.rs_encode(m, NSYM)
            return e.cpu()

        assert torch.equal(one_launch().long(), separate().long()) and torch.equal(dec, detect(rx))
        ts = {one_launch: [], separate: []}
        for fn in ts:  # warm
            for _ in range(20):
                fn()
        for _ in range(REPEATS):
            for fn in ts:
                t0 = time.perf_counter()
                for _ in range(ITERS):
                    fn()
                ts[fn].append((time.perf_counter() - t0) / ITERS * 1e6)
        a, b = statistics.median(ts[one_launch]), statistics.median(ts[separate])
        print(f"step   {kind:4s} {decision:7s} S {S} R {R:3d}: one launch {_spread(ts[one_launch])} us, separate launches "
              f"{_spread(ts[separate])} us per block ({b / a:4.2f} x)", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        _step(sys.argv[2], sys.argv[3])
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for kind, decision in [(k, d) for k in ("vnet", "va") for d in ("running", "path")]:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", kind, decision]
        res = subprocess.run(cmd, capture_output=True, text=True)
        text = (res.stdout.strip() if res.returncode == 0 else
                f"--step {kind} {decision}: exit status {res.returncode}\n{res.stdout}{res.stderr[-2000:]}")
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        if res.returncode != 0:  # a fault, abort or time limit: nothing more is started on the device
            sys.exit(1)


if __name__ == "__main__":
    main()
