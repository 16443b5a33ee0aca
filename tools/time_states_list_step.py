"""The by-word LIST step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_list_f32) against the path step of the same build,
and the lock-step trial engine with decision='list' against the trial-after-trial route (harness.eval_by_word per trial, which takes
the same step with one word per launch).  There is no earlier route for the list rule at these state counts: the numbers say what the
rule costs next to the path rule, not what was gained.

  step   per S, one data block of T = 136 symbols (nsym = 2, list_bytes = 4) for R = 1 / 6 / 256 words, as the by-word evaluation
         issues it: the work of the block and the copy of its error counts to the host, on a host clock around the synchronising copy.
           list step  : mvn_vnet_byword_step_states_list_f32 (dec, enc, nerr) + nerr to the host
           path step  : mvn_vnet_byword_step_states_path_f32 (dec, enc, nerr) + nerr to the host
         The two alternate, REPEATS windows of ITERS blocks each; median and (min .. max) of the windows, microseconds per block.
  trials eval_by_word_batched(decision='list') with 6 and 64 trials of the reference's self-supervised flows at 8 and 64 states
         (goldens G16 L3_selfsup, G17 L6_selfsup: 50 blocks, the golden's iteration counts; trial r = the golden's words with its own
         fresh noise): the lock-step engine against trials._one_trial_at_a_time, alternating, blocks per second.
Every S runs in a child process of its own under `timeout`, so one that hangs ends alone; after a child that fails nothing more is
started on the device.

    python tools/time_states_list_step.py [out.txt]     everything (the table of profiles/states_list_step_time.txt)
    python tools/time_states_list_step.py --step S      one state count's steps (what the children run)
    python tools/time_states_list_step.py --trials S    one state count's trial runs
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_states_step import CHILD_TIMEOUT_S, FLOWS, ITERS, NSYM, REPEATS, WEIGHTS, T, _spread  # noqa: E402  (same words, same windows)

LIST_BYTES = 4


def _step(S):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn

    dev = torch.device("cuda:0")
    L, K = int(np.log2(S)), T - 8 * NSYM
    gen = torch.Generator(device=dev).manual_seed(S)
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    name, tag = WEIGHTS[S]  # weights the reference's trainer produced at this memory length
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    with torch.no_grad():
        for i, p in enumerate(det.parameters()):
            p.copy_(torch.tensor(g[tag % i]).reshape(p.shape))
    front = (*[mvn._lib.ptr(mvn._lib.f32c(p)) for p in det._params()], None)
    list_step = mvn._lib.BywordStep("vnet", "list", T, NSYM, LIST_BYTES, n_states=S, states_list=True)
    path_step = mvn._lib.BywordStep("vnet", "path", T, NSYM, n_states=S, states_path=True)
    for R in (1, 6, 256):
        msg = torch.randint(0, 2, (R, K), generator=gen, device=dev).float()
        rx = mvn.transmit(mvn.rs_encode(msg, NSYM), mvn.estimate_channel(L, 0.2, "time_decay"), 9.0, L, torch.randn(R, T, generator=gen, device=dev))
        dec, enc = torch.empty(R, T, device=dev), torch.empty(R, T, device=dev)
        dec_p = torch.empty(R, T, device=dev)
        nerr = torch.empty(R, dtype=torch.int32, device=dev)
        out = {"dec": (mvn._lib.ptr(dec), T), "enc": (mvn._lib.ptr(enc), T)}
        out_p = {"dec": (mvn._lib.ptr(dec_p), T), "enc": (mvn._lib.ptr(enc), T)}

        def lst():
            list_step(dev, mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, front, out, mvn._lib.ptr(nerr), R, False)
            return nerr.cpu()

        def path():
            path_step(dev, mvn._lib.ptr(rx), T, mvn._lib.ptr(msg), K, front, out_p, mvn._lib.ptr(nerr), R, False)
            return nerr.cpu()

        lst(), path()
        assert torch.equal(dec, dec_p)  # the list step reports the path step's detection
        ts = {lst: [], path: []}
        for fn in ts:  # warm
            for _ in range(20):
                fn()
        for _ in range(REPEATS):
            for fn in ts:
                t0 = time.perf_counter()
                for _ in range(ITERS):
                    fn()
                ts[fn].append((time.perf_counter() - t0) / ITERS * 1e6)
        a, b = (statistics.median(ts[fn]) for fn in (lst, path))
        print(f"step   S {S:3d} R {R:3d}: list step {_spread(ts[lst])} us, path step {_spread(ts[path])} us per block "
              f"(list / path {a / b:4.2f}, + {a - b:5.1f} us)", flush=True)


def _trials(S):
    import numpy as np
    import torch

    from meta_viterbinet_amd import trials

    dev = torch.device("cuda:0")
    name, tag = FLOWS[S]
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    ss_it, _, _, _, _, sub, nsym = [int(v) for v in g[f"{tag}_meta"]]
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    L = int(np.log2(S))
    kw = dict(self_supervised=True, self_supervised_iterations=ss_it, decision="list", list_bytes=LIST_BYTES)
    for R in (6, 64):
        gen = torch.Generator(device=dev).manual_seed(R)
        tx = torch.tensor(g[f"{tag}_tx"], device=dev).float().unsqueeze(0).repeat(R, 1, 1)
        rx = torch.tensor(g[f"{tag}_rx"], device=dev).unsqueeze(0).repeat(R, 1, 1)
        rx = (rx + 0.1 * torch.randn(rx.shape, generator=gen, device=dev)).contiguous()
        N = rx.shape[1]

        def lock_step():
            bank = trials.TrialBank([w0] * R, S, L, dev)
            return trials.eval_by_word_batched(bank, tx, rx, nsym, sub, [trials.TrialDraws(r, dev) for r in range(R)], **kw)

        def one_by_one():
            bank = trials.TrialBank([w0] * R, S, L, dev)
            return trials._one_trial_at_a_time(bank, tx, rx, nsym, sub, [trials.TrialDraws(r, dev) for r in range(R)], np.zeros((R, N)),
                                               None, None, dict(kw), 32)

        assert np.array_equal(lock_step(), one_by_one())  # (also the warm-up of both)
        ts = {lock_step: [], one_by_one: []}
        for _ in range(3):
            for fn in ts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[fn].append(R * N / (time.perf_counter() - t0))
        a, b = statistics.median(ts[lock_step]), statistics.median(ts[one_by_one])
        print(f"trials S {S:3d} {tag} R {R:3d} x {N} blocks, {ss_it} iterations, list: lock-step {_spread(ts[lock_step])} blocks/s, "
              f"trial after trial {_spread(ts[one_by_one])} blocks/s ({a / b:5.1f} x)", flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] in ("--step", "--trials"):
        (_step if sys.argv[1] == "--step" else _trials)(int(sys.argv[2]))
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for what, S in [("--step", S) for S in (4, 8, 32, 64, 128)] + [("--trials", S) for S in sorted(FLOWS)]:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), what, str(S)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        text = res.stdout.strip() if res.returncode == 0 else f"{what} {S}: exit status {res.returncode}\n{res.stdout}{res.stderr[-2000:]}"
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        if res.returncode != 0:  # a fault, abort or time limit: nothing more is started on the device
            sys.exit(1)


if __name__ == "__main__":
    main()
