"""Launch durations of the by-word data step with the list decode (mvn_*_byword_step_list_f32, list_bytes m = 2, 4, 8) against the
path step (mvn_*_byword_step_path_f32) of the same build: warm HIP events around back-to-back launches, median of 5 repeats, for the
ViterbiNet and Viterbi detectors at R = 1, 6, 256 words and T = 136, 512; and one end-to-end pair, harness.eval_by_word over 300
blocks without updates with decision='path' / 'list'.  Every configuration runs in a child process of its own under `timeout`, so
one that hangs ends alone; after a child that fails nothing more is started.

    python tools/time_list_step.py [out.txt]        all configurations (the table of profiles/list_step_time.txt)
    python tools/time_list_step.py --one KIND T R   one configuration (what the children run); KIND vnet | va | e2e
"""
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSYM, ITERS, REPEATS, CHILD_TIMEOUT_S = 2, 200, 5, 120
LIST_BYTES = (2, 4, 8)


def _one(kind, T, R):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn
    from meta_viterbinet_amd.trials import TrialBank

    dev = torch.device("cuda:0")
    g7 = np.load(os.path.join(ROOT, "tests", "golden", "g7_by_word.npz"))
    w = [g7[f"w{i}"] for i in range(6)]
    lib, st = mvn._lib.load(), mvn._lib.current_stream(dev)
    K = T - 8 * NSYM
    gen = torch.Generator(device=dev).manual_seed(1)
    if kind == "e2e":
        N = R
        msg = torch.randint(0, 2, (N, K), generator=gen, device=dev).float()
        rx = mvn.transmit(mvn.rs_encode(msg, NSYM), mvn.estimate_channel(4, 0.2, "time_decay"), 8.0, 4, torch.randn(N, T, generator=gen, device=dev))
        det = mvn.VNETDetector(16, {"train": T, "val": T}).to(dev)
        with torch.no_grad():
            for p, a in zip(det.parameters(), w):
                p.copy_(torch.tensor(a))
        out = []
        for decision in ("path", "list"):
            ser = mvn.eval_by_word(det, msg, rx, 8.0, 0.2, NSYM, 25, decision=decision)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                mvn.eval_by_word(det, msg, rx, 8.0, 0.2, NSYM, 25, decision=decision)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / N * 1e6)
            out.append((statistics.median(ts), int((ser > 0).sum())))
        print(f"eval_by_word {N} blocks x {T}, 8 dB, no updates: path {out[0][0]:6.1f} us per block ({out[0][1]} failed words), "
              f"list (m = {NSYM + 2}) {out[1][0]:6.1f} us per block ({out[1][1]} failed words)", flush=True)
        return
    msg = torch.randint(0, 2, (R, K), generator=gen, device=dev).float()
    rx = mvn.transmit(mvn.rs_encode(msg, NSYM), mvn.estimate_channel(4, 0.2, "time_decay"), 8.0, 4, torch.randn(R, T, generator=gen, device=dev))
    dec, enc = torch.empty(R, T, device=dev), torch.empty(R, T, device=dev)
    lab, nerr = torch.empty(R, T, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    tail = (mvn._lib.ptr(dec), T, None, K, mvn._lib.ptr(enc), T, None, T, mvn._lib.ptr(lab), T, mvn._lib.ptr(nerr), R, T, NSYM, 0, 16, st)
    if kind == "vnet":
        bank = TrialBank([w] * R, 16, 4, dev)
        wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
        head = (mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, *wp, (ctypes.c_int64 * 6)(*([bank.P] * 6)))
        fns = (lib.mvn_vnet_byword_step_path_f32, lib.mvn_vnet_byword_step_list_f32)
    else:
        va = mvn.VADetector(16, 4, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
        pri = va.compute_state_priors(mvn.estimate_channel(4, 0.2, "time_decay")).to(dev).T.contiguous()
        head = (mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, mvn._lib.ptr(pri), 1)
        fns = (lib.mvn_va_byword_step_path_f32, lib.mvn_va_byword_step_list_f32)

    def ev(fn, *extra):
        args = head + tail[:-1] + extra + tail[-1:]
        for _ in range(20):
            assert fn(*args) == 0
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                fn(*args)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / ITERS * 1e3)
        return statistics.median(ts), int((nerr > 0).sum())

    t_path, bad_path = ev(fns[0])
    cols = []
    for m in LIST_BYTES:
        t_list, bad_list = ev(fns[1], m, None, T, None)  # (no delta, no choice: what eval_by_word asks for)
        cols.append(f"m = {m}: {t_list:7.1f} us ({t_list / t_path:4.2f} x, {bad_list} words with errors)")
    print(f"{kind:4s} T {T:4d} R {R:3d}: path step {t_path:7.1f} us ({bad_path} words with errors) | list step " + ", ".join(cols), flush=True)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--one":
        _one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    configs = [(kind, T, R) for kind in ("vnet", "va") for T in (136, 512) for R in (1, 6, 256)] + [("e2e", 136, 300)]
    for kind, T, R in configs:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--one", kind, str(T), str(R)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        line = res.stdout.strip() if res.returncode == 0 else f"{kind} T {T} R {R}: exit status {res.returncode}\n{res.stderr[-2000:]}"
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        if res.returncode != 0:  # a fault, abort or time limit: nothing more is started on the device
            sys.exit(1)


if __name__ == "__main__":
    main()
