"""The ViterbiNet training kernels' gradient against torch autograd in float64, per case and tensor of tests/vnet_grad_cases.py:
the kernel's largest elementwise error and stock float32 torch's (CPU autograd), both relative to the tensor's largest entry, and
the kernel's error in units of max(d32, floor) -- the figure tests/test_gpu_vnet_grad.py holds below its margin of 8.  Runs the
tests' own assertions on the way and lists the cases that failed them.
usage: vnet_train_gradients.py [--out FILE]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vnet_grad_cases as G  # noqa: E402

out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda:0")
rows, failed = [], []


def attempt(name, check):
    try:
        check()
    except AssertionError as e:
        failed.append(f"{name}: {str(e).splitlines()[0] if str(e) else 'assertion'}")


for name in G.ONLINE_NAMES:
    attempt(name, lambda: G.check_first_iteration(G.ONLINE[name], dev, True, G.MARGIN_KERNEL, rows))
    if G.ONLINE[name]["second"]:
        attempt(name + " iter 2", lambda: G.check_second_iteration(G.ONLINE[name], dev, True, G.MARGIN_KERNEL, None, rows))
for S in G.WORDS_STATES:
    attempt(f"S{S} train_words", lambda: G.check_words(S, dev, True, G.MARGIN_KERNEL, rows))
for name in G.MAML_NAMES:
    attempt("maml " + name, lambda: G.check_maml(G.MAML[name], dev, True, G.MARGIN_KERNEL, rows))
lines = [f"ViterbiNet training kernels on {torch.cuda.get_device_name(dev)}: gradient of one iteration (2 exp_avg after one Adam step with",
         "beta1 = 0.5; 'iter 2': 2 m2 - m1; 'maml': the meta-gradient of one step) against torch autograd in float64.  d32: stock float32",
         "torch (CPU autograd) against the same referee; floor: 2^-23 max|g64|; all errors are the largest over the",
         "tensor's elements.  The tests' margin is 8.",
         "",
         f"{'case':40s} {'tensor':6s} {'max|g64|':>10s} {'torch f32 / max':>16s} {'kernel / max':>13s} {'torch f32 / unit':>17s} {'kernel / unit':>14s}"]
for label, tensor, top, d32, err, ratio in rows:
    unit = max(d32, 2.0 ** -23 * top)
    rel = (lambda x: x / top) if top > 0 else (lambda x: 0.0)
    lines.append(f"{label:40s} {tensor:6s} {top:10.3e} {rel(d32):16.3e} {rel(err):13.3e} {(d32 / unit if unit else 0.0):17.3f} {ratio:14.3f}")
worst = {}
for label, tensor, top, d32, err, ratio in rows:
    kind = "maml" if label.startswith("maml") else "online"
    worst[(kind, tensor)] = max(worst.get((kind, tensor), 0.0), ratio)
lines += ["", "largest kernel / unit per tensor: " + ", ".join(f"{k} {t} {w:.2f}" for (k, t), w in worst.items())]
lines += ["cases that failed an assertion: " + ("none" if not failed else "")] + failed
print("\n".join(lines[-2 - len(failed):]))
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
