"""The meta-learning step at 32, 64 and 128 states: the one-launch kernel (mvn_vnet_maml_train_ws_f32: maml_train_kernel<32, false> or
its chunked form at 32 states, maml_train_kernel<64 | 128, false> above) against the two autograd routes of the same build, and the
by-word evaluation of golden G21's flows with the kernel against the route it took before.

  step   per S, first and second order, words of T = 136 symbols, W = 1 support word, microseconds per step between HIP events:
           kernel  : OnlineTrainer.maml_training, STEPS steps per launch
           graphed : meta.GraphedMetaStep, one replay per step (what harness.eval_by_word took above 32 states)
           eager   : meta.meta_train_loop, torch autograd with create_graph
         after a warm-up, REPEATS windows each, the three alternating; median and (min .. max) of the windows.
  flow   harness.eval_by_word over the 50 blocks of G21's L6_meta / L7_meta (64 / 128 states: 6 whole-word iterations per block,
         2 x 4 second-order steps every 5 blocks, the global generator's draws) with hip_meta=True against hip_meta=False
         (GraphedMetaStep), alternating, blocks per second on a host clock.
Every S runs in a child process of its own under `timeout`; after a child that fails nothing more is started on the device.

    python tools/time_maml_states.py [out.txt]     everything (the table of profiles/maml_states_time.txt)
    python tools/time_maml_states.py --step S      one state count's steps (what the children run)
    python tools/time_maml_states.py --flow S      one state count's flow
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, STEPS, REPEATS, CHILD_TIMEOUT_S = 136, 40, 7, 240
# (golden, key of weight i, key of the received words): weights the reference's own trainer produced at that channel memory
INPUTS = {32: ("g16_by_word_other_state_counts", "L5_meta_w0_%d", "g16_by_word_other_state_counts", "L5_meta_rx"),
          64: ("g17_by_word_64_128_states", "L6_selfsup_w0_%d", "g21_by_word_meta_64_128_states", "L6_meta_rx"),
          128: ("g17_by_word_64_128_states", "L7_selfsup_w0_%d", "g21_by_word_meta_64_128_states", "L7_meta_rx")}


def _spread(v):
    return f"{statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})"


def _golden(name):
    import numpy as np

    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _detector(S, w, dev):
    import torch

    import meta_viterbinet_amd as mvn

    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w):
            p.copy_(torch.as_tensor(a).reshape(p.shape))
    return det


def _step(S):
    import ctypes

    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn

    dev = torch.device("cuda:0")
    L = int(np.log2(S))
    wname, wkey, rname, rkey = INPUTS[S]
    w = [_golden(wname)[wkey % i] for i in range(6)]
    rxw = torch.tensor(_golden(rname)[rkey][:10], device=dev)
    txw = torch.randint(0, 2, (10, T), generator=torch.Generator(device=dev).manual_seed(S), device=dev).float()
    meta = mvn.META_VNETDetector(S, {"train": T, "val": T})
    sup = (torch.arange(STEPS, device=dev) % 8).reshape(-1, 1)
    qry = sup.reshape(-1) + 1
    name = ctypes.create_string_buffer(160)
    for MAML in (False, True):
        dets = [_detector(S, w, dev) for _ in range(3)]
        trs = [mvn.OnlineTrainer(d, L) for d in dets]
        ws_bytes = trs[0]._workspace(S, dev).numel()
        mvn._lib.load().mvn_vnet_train_kernel_name(2 if MAML else 1, 0, T, 1, S, ws_bytes, name, 160)
        graphed = mvn.GraphedMetaStep(dets[1], meta, trs[1], 1, T, 0.1, MAML)

        def kernel():
            trs[0].maml_training(rxw, txw, sup, qry, 0.1, MAML)

        def graph():
            for k in range(STEPS):
                graphed(rxw, txw, sup[k], qry[k:k + 1])

        def eager():
            for k in range(STEPS):
                mvn.meta_train_loop(dets[2], meta, trs[2], rxw, txw, sup[k], qry[k:k + 1], 0.1, MAML)

        ts = {kernel: [], graph: [], eager: []}
        for fn in ts:  # warm
            fn()
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for fn in ts:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[fn].append(e0.elapsed_time(e1) * 1e3 / STEPS)
        a, b, c = (statistics.median(ts[fn]) for fn in (kernel, graph, eager))
        print(f"step S {S:3d} {'second' if MAML else 'first '} order, T {T} W 1: kernel {_spread(ts[kernel])} us per step [{name.value.decode()}], "
              f"graphed replay {_spread(ts[graph])} us ({b / a:5.1f} x), eager autograd {_spread(ts[eager])} us ({c / a:5.1f} x)", flush=True)


def _flow(S):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn

    dev = torch.device("cuda:0")
    L = int(np.log2(S))
    tag = f"L{L}_meta"
    g = _golden("g21_by_word_meta_64_128_states")
    ss_it, meta_it, j_num, meta_sub, _, subframes, nsym = [int(v) for v in g[f"{tag}_meta"]]
    tx, rx = torch.tensor(g[f"{tag}_tx"], device=dev).float(), torch.tensor(g[f"{tag}_rx"], device=dev)
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]

    def run(hip_meta):
        torch.manual_seed(0)
        det = _detector(S, w0, dev)
        tr = mvn.OnlineTrainer(det, L)
        return mvn.eval_by_word(det, tx, rx, 9.0, 0.2, nsym, subframes, self_supervised=True, self_supervised_iterations=ss_it,
                                online_trainer=tr, online_meta=True, meta_detector=mvn.META_VNETDetector(S, {"train": T, "val": T}),
                                meta_lr=0.1, MAML=True, window_size=1, meta_train_iterations=meta_it, meta_j_num=j_num,
                                meta_subframes=meta_sub, meta_style_online_training=True, hip_meta=hip_meta)

    ts = {True: [], False: []}
    same = np.array_equal(run(True), run(False))  # (also the warm-up of both)
    for _ in range(5):
        for hip_meta in ts:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(hip_meta)
            torch.cuda.synchronize()
            ts[hip_meta].append(len(rx) / (time.perf_counter() - t0))
    a, b = statistics.median(ts[True]), statistics.median(ts[False])
    print(f"flow S {S:3d} {tag}, {len(rx)} blocks, {ss_it} iterations per block, {meta_it} x <= {j_num} second-order steps every {meta_sub} blocks: "
          f"hip_meta=True {_spread(ts[True])} blocks/s, hip_meta=False (graphed) {_spread(ts[False])} blocks/s ({a / b:4.2f} x); "
          f"ser_by_word {'identical' if same else 'differs'}", flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] in ("--step", "--flow"):
        (_step if sys.argv[1] == "--step" else _flow)(int(sys.argv[2]))
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for what, S in [("--step", S) for S in (32, 64, 128)] + [("--flow", S) for S in (64, 128)]:
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
