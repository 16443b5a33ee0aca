"""The trial axis of the meta-learning step at 64 and 128 states: ONE mvn_vnet_maml_train_states_trials_f32 call for R trials
(maml_train_states_trials_kernel<64 | 128>, a workgroup per trial) against R back-to-back mvn_vnet_maml_train_ws_f32 calls on the
same data in the same build, and the lock-step engine (trials.eval_by_word_batched) on golden G21's flows against the
trial-after-trial route of the same build.

  call   per S, first and second order, words of T = 136 symbols, W = 1 support word, R = 2 / 6 / 64 / 256 / 300 trials of 8 steps
         (G21's updates) and of 200 steps (the reference's 20 x 10), milliseconds between HIP events:
           trials   : one call of the new entry point (one launch, gridDim.y = R)
           one by one : R calls of mvn_vnet_maml_train_ws_f32 on one stream (maml_train_kernel<64 | 128, false>)
         alternating after a warm-up; median and (min .. max) of the windows (the long one-by-one windows are repeated less often).
         Both start from the same state: after the first window every trial's weights are compared bit for bit.
  flow   trials.eval_by_word_batched over the 50 blocks of G21's L6_meta / L7_meta (64 / 128 states: 6 whole-word iterations per
         block, 2 x <= 4 second-order steps every 5 blocks) with R = 2 / 6 / 64 trials -- the golden's words and copies with fresh
         noise -- default arguments (the engine for R >= trials.META_TRIAL_AXIS_MIN_R) against meta_trial_axis=True and
         meta_trial_axis=False (trial after trial), alternating, blocks per second (R x 50 / seconds) on a host clock.
  default  the same flow with default arguments only, written without the keyword so that it also runs on a tree that has none.
Every S runs in a child process of its own under `timeout`; after a child that fails nothing more is started on the device.

    python tools/time_maml_states_trials.py [out.txt]     everything (the table of profiles/maml_states_trials_time.txt)
    python tools/time_maml_states_trials.py --call S      one state count's calls (what the children run)
    python tools/time_maml_states_trials.py --flow S      one state count's flow
    python tools/time_maml_states_trials.py --default S   one state count's flow, default arguments only
"""
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, W, CHILD_TIMEOUT_S = 136, 1, 420
TRIALS, STEPS, FLOW_TRIALS = (2, 6, 64, 256, 300), (8, 200), (2, 6, 64)
META_LR, LR, B1, B2, EPS = 0.1, 1e-3, 0.9, 0.999, 1e-8
INPUTS = {64: ("g17_by_word_64_128_states", "L6_selfsup_w0_%d", "g21_by_word_meta_64_128_states", "L6_meta_rx"),
          128: ("g17_by_word_64_128_states", "L7_selfsup_w0_%d", "g21_by_word_meta_64_128_states", "L7_meta_rx")}


def _spread(v, fmt="%.2f"):
    return f"{fmt % statistics.median(v)} ({fmt % min(v)} .. {fmt % max(v)})"


def _golden(name):
    import numpy as np

    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _call(S):
    import numpy as np
    import torch

    import meta_viterbinet_amd as mvn
    from meta_viterbinet_amd import _lib
    from meta_viterbinet_amd.trials import TRIAL_DTYPE, param_offsets

    dev = torch.device("cuda:0")
    lib = _lib.load()
    wname, wkey, rname, rkey = INPUTS[S]
    w = [_golden(wname)[wkey % i] for i in range(6)]
    rxw = torch.tensor(_golden(rname)[rkey][:10], device=dev).contiguous()
    txw = torch.randint(0, 2, (10, T), generator=torch.Generator(device=dev).manual_seed(S), device=dev).float()
    lab = mvn.calculate_states(int(np.log2(S)), txw).reshape(10, T).to(torch.int32).contiguous()
    base = torch.cat([torch.as_tensor(a).reshape(-1) for a in w]).to(dev)
    off, P = param_offsets(S), base.numel()
    stream = _lib.current_stream(dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(1)
    for second in (0, 1):
        for n in STEPS:
            sup = (torch.arange(n, device=dev, dtype=torch.int32) % 8).contiguous()
            qry = (sup + 1).contiguous()
            for R in TRIALS:
                start = (base + 0.01 * torch.randn((R, P), generator=gen, device=dev)).contiguous()
                # two copies of the trials' state: [0] for the one call, [1] for the R calls
                th = [start.clone() for _ in range(2)]
                m, v = [torch.zeros_like(start) for _ in range(2)], [torch.zeros_like(start) for _ in range(2)]
                desc = np.zeros(R, TRIAL_DTYPE)
                rows = th[0].data_ptr() + 4 * P * np.arange(R, dtype=np.uint64)
                six = rows[:, None] + (4 * off[:6]).astype(np.uint64)[None, :]
                desc["y"], desc["labels"], desc["idx"], desc["query_idx"] = rxw.data_ptr(), lab.data_ptr(), sup.data_ptr(), qry.data_ptr()
                desc["w_in"], desc["w_out"] = six, six
                desc["adam_m"] = m[0].data_ptr() + 4 * P * np.arange(R, dtype=np.uint64)
                desc["adam_v"] = v[0].data_ptr() + 4 * P * np.arange(R, dtype=np.uint64)
                desc["b1pow"], desc["b2pow"], desc["n"] = 1.0, 1.0, n  # (every window as if from step 0: the time does not depend on it)
                d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
                ptrs = [[ctypes.c_void_p(th[1].data_ptr() + 4 * (P * r + int(off[a]))) for a in range(6)] for r in range(R)]
                mp = [ctypes.c_void_p(m[1].data_ptr() + 4 * P * r) for r in range(R)]
                vp = [ctypes.c_void_p(v[1].data_ptr() + 4 * P * r) for r in range(R)]

                def trials_call():
                    rc = lib.mvn_vnet_maml_train_states_trials_f32(_lib.ptr(d), R, T, W, META_LR, second, LR, B1, B2, EPS, S, stream)
                    _lib.check(rc, "mvn_vnet_maml_train_states_trials_f32")

                def one_by_one():
                    for r in range(R):
                        rc = lib.mvn_vnet_maml_train_ws_f32(_lib.ptr(rxw), _lib.ptr(lab), T, _lib.ptr(sup), W, _lib.ptr(qry), n, *ptrs[r],
                                                            mp[r], vp[r], 0, META_LR, second, LR, B1, B2, EPS, None, S, None, 0, None, stream)
                        _lib.check(rc, "mvn_vnet_maml_train_ws_f32")

                def timed(fn):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                trials_call()  # the warm-up, and the comparison
                one_by_one()
                torch.cuda.synchronize()
                same = all(torch.equal(a[0], a[1]) for a in (th, m, v))
                long = R * n > 2000  # a one-by-one window of seconds: fewer of them
                ts = {trials_call: [], one_by_one: []}
                for k in range(7):
                    ts[trials_call].append(timed(trials_call))
                    if k < (2 if long else 7):
                        ts[one_by_one].append(timed(one_by_one))
                a, b = statistics.median(ts[trials_call]), statistics.median(ts[one_by_one])
                print(f"call S {S:3d} {'second' if second else 'first '} order, T {T} W {W}, {n:3d} steps, R {R:3d} ({-(-R // cus)} round{'s' if R > cus else ''} "
                      f"of {cus} CUs): trials {_spread(ts[trials_call])} ms = {a * 1e3 / n:7.1f} us per step of all trials, one by one "
                      f"{_spread(ts[one_by_one])} ms ({b / a:6.1f} x, {len(ts[one_by_one])} windows); results {'identical' if same else 'DIFFER'}",
                      flush=True)
                if not same:
                    sys.exit(2)


def _flow_inputs(S, R, dev):
    import numpy as np
    import torch

    L = int(np.log2(S))
    tag = f"L{L}_meta"
    g = _golden("g21_by_word_meta_64_128_states")
    ss_it, meta_it, j_num, meta_sub, _, subframes, nsym = [int(x) for x in g[f"{tag}_meta"]]
    tx1, rx1 = torch.tensor(g[f"{tag}_tx"], device=dev).float(), torch.tensor(g[f"{tag}_rx"], device=dev)
    gen = torch.Generator(device=dev).manual_seed(S)
    rx = torch.stack([rx1] + [rx1 + 0.15 * torch.randn(rx1.shape, generator=gen, device=dev) for _ in range(R - 1)]).contiguous()
    tx = tx1.unsqueeze(0).repeat(R, 1, 1).contiguous()
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    kw = dict(self_supervised=True, self_supervised_iterations=ss_it, online_meta=True, meta_lr=META_LR, MAML=True, window_size=1,
              meta_train_iterations=meta_it, meta_j_num=j_num, meta_subframes=meta_sub, meta_style_online_training=True)
    return tag, L, w0, tx, rx, nsym, subframes, kw, (ss_it, meta_it, j_num, meta_sub)


def _flow(S, default_only=False):
    import numpy as np
    import torch

    from meta_viterbinet_amd.trials import TrialBank, TrialDraws, eval_by_word_batched

    dev = torch.device("cuda:0")
    for R in FLOW_TRIALS:
        tag, L, w0, tx, rx, nsym, subframes, kw, (ss_it, meta_it, j_num, meta_sub) = _flow_inputs(S, R, dev)

        def run(more):
            bank = TrialBank([w0] * R, S, L, dev)
            ser = eval_by_word_batched(bank, tx, rx, nsym, subframes, [TrialDraws(100 + r, dev) for r in range(R)], **kw, **more)
            torch.cuda.synchronize()
            return ser, bank.theta.clone()

        routes = {"default": {}} if default_only else {"default": {}, "meta_trial_axis=True": dict(meta_trial_axis=True),
                                                       "meta_trial_axis=False": dict(meta_trial_axis=False)}
        first = {name: run(more) for name, more in routes.items()}  # (also the warm-up of every route)
        same = all(np.array_equal(first["default"][0], s) and torch.equal(first["default"][1], t) for s, t in first.values())
        ts = {name: [] for name in routes}
        for _ in range(5):
            for name, more in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(more)
                ts[name].append(R * rx.shape[1] / (time.perf_counter() - t0))
        text = ", ".join(f"{name} {_spread(v, '%.0f')}" for name, v in ts.items())
        ratio = "" if default_only else (f"; engine / trial after trial "
                                         f"{statistics.median(ts['meta_trial_axis=True']) / statistics.median(ts['meta_trial_axis=False']):.2f} x")
        print(f"flow S {S:3d} {tag}, R {R:2d} x {rx.shape[1]} blocks, {ss_it} iterations per block, {meta_it} x <= {j_num} second-order steps every "
              f"{meta_sub} blocks, blocks/s: {text}{ratio}; rows {'identical' if same else 'DIFFER'}", flush=True)
        if not same:
            sys.exit(2)


def main():
    modes = {"--call": _call, "--flow": _flow, "--default": lambda S: _flow(S, True)}
    if len(sys.argv) == 3 and sys.argv[1] in modes:
        modes[sys.argv[1]](int(sys.argv[2]))
        return
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for what, S in [("--call", S) for S in (64, 128)] + [("--flow", S) for S in (64, 128)]:
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
