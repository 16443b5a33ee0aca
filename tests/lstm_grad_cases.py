"""Shared by tests/test_lstm_grad_host.py, tests/test_gpu_lstm_grad.py and tools/lstm_train_gradients.py (no tests of its own):
the per-element gradient of LSTMOnlineTrainer (lstm_train_kernel behind it on the GPU) against torch autograd in float64.

The readout.  Adam's first moment gives the gradient with no optimizer in the way: from a zero state with betas = (0.5, 0.999) one
iteration leaves exp_avg = 0.5 * 0 + 0.5 * g, so g = 2 * exp_avg exactly (a power of two), for all 795 138 parameters in
parameters() order, and exp_avg_sq = (1 - beta2) g^2 to float32 rounding.  With lr = 0.02 that step moves every weight by 0.02
sign(g), about a third of its scale (step_size = lr / (1 - 0.5), m / (sqrt(v) / sqrt(1 - beta2) + eps) = 0.5 g / |g|), and a second
iteration leaves m2 = 0.5 m1 + 0.5 g2: g2 = 2 m2 - m1 with m1 from a separate one-iteration run (split calls are bit-identical,
tests/test_gpu_lstm_train.py), compared with the float64 gradient at the route's OWN weights after step 1, so only iteration 2's
gradient is under test.  One SGD step with lr = 64 (a power of two: lr * g is exact) must give w1 = fl(w0 - 64 g) to 1 ulp (fma
contraction), which pins p -= lr g per element.

The bound is measured against the reference, not against the code under test: per case and tensor d32 = max |g32 - g64| of stock
float32 torch autograd on the CPU, and
    bound = MARGIN * max(d32, 2^-23 max |g64|)
elementwise on the whole tensor; MARGIN = 8 for the kernel (its expf-based sigmoid and tanh, ascending chains of T fmaf where torch
sums in blocks), 2 for the autograd route (float32 torch on the same formulas).  The smallest defect the table aims at, one time
step dropped from a weight gradient at T = 256, is about 4e-3 of the tensor's largest entry; d32 is 2e-7 ... 2e-6 of it."""
import os

import numpy as np
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L
from test_lstm_host import g18_weights
from test_lstm_train_host import check_losses, default_init_weights, detector_with, draw_batches

NAMES = ["W_ih0", "W_hh0", "b_ih0", "b_hh0", "W_ih1", "W_hh1", "b_ih1", "b_hh1", "fc_W", "fc_b"]
SIZES = [int(np.prod(s)) for s in L.PARAM_SHAPES]
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)])
BETAS = (0.5, 0.999)
LR = 0.02        # Adam: every weight moves by 0.02 in step 1
SGD_LR = 64.0
MARGIN_KERNEL, MARGIN_AUTOGRAD = 8.0, 2.0
SHARE_TENSORS = (4, 5, 8)  # W_ih1, W_hh1, fc_W: where 99 % of the referee's entries must lie above the bound
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name, T, idx=None, weights="init", zero=(), second=False):
    """idx: None (the whole word) or the positions of iteration 1 (and 2), [1 or 2, M]; zero: tensors whose gradient is exactly
    zero; second: the case also checks the second iteration's gradient."""
    if idx is not None:
        idx = torch.as_tensor(np.asarray(idx), dtype=torch.int32).reshape(-1, np.asarray(idx).shape[-1])
    return dict(name=name, T=T, idx=idx, weights=weights, zero=tuple(zero), second=second)


def _table():
    W_HH = (1, 5)  # W_hh0, W_hh1 multiply h(t - 1): no gradient when only t = 0 is in the loss
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(256))
    drawn136 = draw_batches(136, 2, 32, 138)  # (seeds 136 and 137 leave 98.9 % of W_hh1 above the bound: stock float32 is at 10-16 floors there)
    # Where the loss sees the first three steps only, the -100 padding of the window saturates layer 0 under the default initialisation
    # (z = -100 (w0 + w1 + w2), sigma 6) and 20-40 % of W_ih1's gradient d1 (x) h0 lies below the bound: those cases take W_ih0 / 16.
    out = [_case(f"whole_T{T}", T, weights="init_in16" if T <= 3 else "init", zero=W_HH if T == 1 else (), second=T in (2, 256))
           for T in (1, 2, 3, 4, 5, 40, 136, 255, 256)]
    out += [_case("one_T256_p255", 256, [[255]]), _case("one_T256_p0", 256, [[0]], weights="init_in16", zero=W_HH),
            _case("one_T256_p128", 256, [[128]]),
            _case("dup_T136", 136, [[7, 7, 7, 135]]), _case("dup_T255", 255, [[254, 0, 254]]), _case("dup_T5", 5, [[4, 4]]),
            _case("drawn_T136_M32", 136, drawn136, second=True), _case("drawn_T40_M32", 40, draw_batches(40, 1, 32, 40)),
            _case("perm_T256_M256", 256, perm.reshape(1, 256)), _case("drawn_T1_M1", 1, [[0]], weights="init_in16", zero=W_HH)]
    # the T = 136 cases once more from G18's trained weights (saturated gates, int8 grid)
    out += [_case("whole_T136_g18", 136, weights="g18"), _case("dup_T136_g18", 136, [[7, 7, 7, 135]], weights="g18"),
            _case("drawn_T136_M32_g18", 136, drawn136, weights="g18", second=True)]
    return out


CASES = {c["name"]: c for c in _table()}
CASE_NAMES = list(CASES)
SECOND_NAMES = [n for n in CASE_NAMES if CASES[n]["second"]]
DUPLICATE_NAMES = [n for n in CASE_NAMES if n.startswith("dup_")]


def word(T):
    """One word, seeded by T: (bits int64 [1, T], rx float32 [1, T])."""
    rng = np.random.RandomState(T)
    bits = rng.randint(0, 2, (1, T))
    rx = ((1 - 2 * bits) + 0.4 * rng.randn(1, T)).astype(np.float32)
    return bits, rx


_WEIGHTS = {}


def weights(kind):
    if kind not in _WEIGHTS:
        if kind == "g18":
            _WEIGHTS[kind] = g18_weights(np.load(os.path.join(_GOLDEN, "g18_lstm.npz")))
        else:
            ws = default_init_weights(3)
            if kind == "init_in16":
                ws[0] = ws[0] / np.float32(16)
            _WEIGHTS[kind] = ws
    return _WEIGHTS[kind]


def torch_gradient(ws, bits, rx, sel, dtype):
    """torch.nn.LSTM + Linear in `dtype` on the CPU, L.sliding_windows, cross_entropy over the selection (None: the whole word),
    torch.autograd.grad: (ten float64 arrays, loss)."""
    lstm = torch.nn.LSTM(L.INPUT_SIZE, L.HIDDEN_SIZE, L.NUM_LAYERS, batch_first=True).to(device="cpu", dtype=dtype)
    fc = torch.nn.Linear(L.HIDDEN_SIZE, L.N_CLASSES).to(device="cpu", dtype=dtype)
    params = list(lstm.parameters()) + list(fc.parameters())
    with torch.no_grad():
        for p, w in zip(params, ws):
            p.copy_(torch.from_numpy(np.asarray(w)).to(dtype))
    y, lab = torch.from_numpy(np.asarray(rx)).to(dtype), torch.from_numpy(np.asarray(bits)).long()[0]
    logits = fc(lstm(L.sliding_windows(y))[0]).reshape(-1, L.N_CLASSES)
    if sel is None:
        loss = torch.nn.functional.cross_entropy(logits, lab)
    else:
        sel = torch.as_tensor(np.asarray(sel)).long()
        loss = torch.nn.functional.cross_entropy(logits[sel], lab[sel])
    grads = torch.autograd.grad(loss, params)
    return [g.double().numpy() for g in grads], float(loss.detach())


def reference(ws, bits, rx, sel):
    """dict(g64, loss64, d32 [10], floor [10]): the float64 referee and stock float32 torch's distance from it."""
    g64, loss64 = torch_gradient(ws, bits, rx, sel, torch.float64)
    g32, _ = torch_gradient(ws, bits, rx, sel, torch.float32)
    d32 = np.array([np.abs(a - b).max() for a, b in zip(g32, g64)])
    floor = np.array([2.0 ** -23 * np.abs(b).max() for b in g64])
    return dict(g64=g64, loss64=loss64, d32=d32, floor=floor)


_REFERENCE = {}


def reference_of(case):
    """The referee of the case's FIRST iteration, computed once per process and left unchanged."""
    if case["name"] not in _REFERENCE:
        bits, rx = word(case["T"])
        _REFERENCE[case["name"]] = reference(weights(case["weights"]), bits, rx, None if case["idx"] is None else case["idx"][0])
    return _REFERENCE[case["name"]]


def split(flat):
    """exp_avg / exp_avg_sq [795138] -> ten arrays in parameters() order."""
    flat = flat.detach().cpu().numpy()
    return [flat[OFFSETS[k]:OFFSETS[k + 1]].reshape(L.PARAM_SHAPES[k]) for k in range(10)]


def run(case, device, use_kernel, n=1, optimizer_type="Adam", lr=LR):
    """n iterations of the case from a zero optimizer state: dict(w, m, v: ten float32 arrays each; loss [n]; tr)."""
    bits, rx = word(case["T"])
    det = detector_with(weights(case["weights"]), device)
    tr = mvn.LSTMOnlineTrainer(det, lr=lr, betas=BETAS, use_kernel=use_kernel, optimizer_type=optimizer_type)
    assert tr.kernel_route(case["T"]) == bool(use_kernel and torch.device(device).type == "cuda")
    tx, y = torch.from_numpy(bits.astype(np.float32)).to(device), torch.from_numpy(rx).to(device)
    idx = None if case["idx"] is None else case["idx"][:n]
    assert idx is None or idx.shape[0] == n
    loss = tr.online_training(tx, y, iterations=n, batch_idx=idx, full_word=idx is None, return_loss=True)
    tr.check_status()
    assert tr.step == n
    return dict(w=[p.detach().cpu().numpy().copy() for p in tr.params], m=split(tr.exp_avg), v=split(tr.exp_avg_sq),
                loss=loss.cpu().numpy(), tr=tr)


def readout(run1):
    """The gradient of a one-iteration Adam run: 2 * exp_avg, exact in float32."""
    return [np.float32(2.0) * m for m in run1["m"]]


def bounds(ref, margin):
    return margin * np.maximum(ref["d32"], ref["floor"])


def compare(label, g, ref, margin, rows=None):
    """Element by element |g - g64| <= margin * max(d32, floor) for the ten tensors; prints every figure before it asserts and
    appends (label, tensor, max |g64|, d32, worst error, error / max(d32, floor)) to rows."""
    bad = []
    for k in range(10):
        err = np.abs(np.asarray(g[k], np.float64) - ref["g64"][k])
        unit = max(ref["d32"][k], ref["floor"][k])
        worst, top = float(err.max()), float(np.abs(ref["g64"][k]).max())
        ratio = worst / unit if unit > 0 else (0.0 if worst == 0 else float("inf"))
        print(f"{label:26s} {NAMES[k]:6s} max|g64| {top:9.3e}  d32 {ref['d32'][k]:9.3e}  error {worst:9.3e}  error / max(d32, floor) {ratio:7.3f}")
        if rows is not None:
            rows.append((label, NAMES[k], top, float(ref["d32"][k]), worst, ratio))
        if not np.all(err <= margin * unit):
            bad.append((NAMES[k], ratio, int((err > margin * unit).sum())))
    assert not bad, f"{label}: (tensor, error / max(d32, floor), elements outside) {bad}, margin {margin}"


def check_zero(case, g, ref):
    for k in case["zero"]:
        assert not ref["g64"][k].any(), (case["name"], NAMES[k])  # the case is what it claims to be
    for k in range(10):  # element by element: e.g. the forget gate's rows at t = 0, where c(t - 1) = 0
        assert not np.asarray(g[k])[ref["g64"][k] == 0].any(), f"{case['name']}: {NAMES[k]} must be exactly zero where the referee is"


def check_second_moment(case, g, v, kernel):
    """exp_avg_sq within 4 ulp of float32(1 - beta2) * g * g.  beta2 crosses the C ABI as a float and adam1 forms 1.0f - beta2, which
    is exact (0.0009999871); torch.optim forms 1 - beta2 in Python's double and rounds that (0.001).  Each route is held to its own
    constant; the two differ by 1.3e-5 of exp_avg_sq."""
    c = np.float32(1.0) - np.float32(BETAS[1]) if kernel else np.float32(1.0 - BETAS[1])
    for k in range(10):
        want = (c * g[k]) * g[k]
        assert want.dtype == np.float32
        off = np.abs(v[k].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"{case['name']:26s} {NAMES[k]:6s} exp_avg_sq: {off.max():.2f} ulp")
        assert off.max() <= 4, (case["name"], NAMES[k], float(off.max()))


def check_sgd(case, g, device, use_kernel):
    """One SGD step with lr = 64: w1 = fl(w0 - 64 g) to 1 ulp of max(|w0|, |w1|)."""
    r = run(case, device, use_kernel, optimizer_type="SGD", lr=SGD_LR)
    for k, w0 in enumerate(weights(case["weights"])):
        want = w0 - np.float32(SGD_LR) * g[k]
        ulp = np.spacing(np.maximum(np.abs(w0), np.abs(want))).astype(np.float64)
        off = np.abs(r["w"][k].astype(np.float64) - want.astype(np.float64)) / ulp
        print(f"{case['name']:26s} {NAMES[k]:6s} SGD step: {off.max():.2f} ulp")
        assert off.max() <= 1, (case["name"], NAMES[k], float(off.max()))
    assert not r["tr"].exp_avg.any() and not r["tr"].exp_avg_sq.any()  # SGD touches neither
    return r


def check_first_iteration(case, device, use_kernel, margin, rows=None):
    """Every per-case assertion on the first iteration; returns (the one-iteration run, its gradient)."""
    ref = reference_of(case)
    r1 = run(case, device, use_kernel)
    g = readout(r1)
    compare(case["name"], g, ref, margin, rows)
    check_zero(case, g, ref)
    for bi, bh in ((2, 3), (6, 7)):  # b_ih and b_hh of a layer share one gradient
        assert np.array_equal(g[bi].view(np.uint32), g[bh].view(np.uint32)), (case["name"], NAMES[bi])
    check_losses(r1["loss"], np.array([ref["loss64"]]))
    check_second_moment(case, g, r1["v"], r1["tr"].kernel_route(case["T"]))
    check_sgd(case, g, device, use_kernel)
    return r1, g


def check_second_iteration(case, device, use_kernel, margin, r1=None, rows=None):
    """g2 = 2 m2 - m1 against the float64 gradient at the route's own weights after step 1."""
    r1 = run(case, device, use_kernel) if r1 is None else r1
    moved = np.concatenate([np.abs(a - b).reshape(-1) for a, b in zip(r1["w"], weights(case["weights"]))])
    print(f"{case['name']}: step 1 moved {np.mean(moved > 0.019):.3f} of the weights by lr")
    assert np.mean(moved > 0.019) > 0.5  # (all but those with |g| ~ eps or 0), so stale copies of them are far off
    r2 = run(case, device, use_kernel, n=2)
    bits, rx = word(case["T"])
    ref2 = reference(r1["w"], bits, rx, None if case["idx"] is None else case["idx"][1])
    g2 = [2.0 * m2.astype(np.float64) - m1.astype(np.float64) for m1, m2 in zip(r1["m"], r2["m"])]
    assert np.array_equal(r2["loss"][:1].view(np.uint32), r1["loss"].view(np.uint32))
    compare(case["name"] + " iter 2", g2, ref2, margin, rows)
    check_losses(r2["loss"][1:], np.array([ref2["loss64"]]))
    return r2


def share_above_bound(ref, margin, k):
    """Fraction of tensor k's non-zero referee entries larger in magnitude than the bound (None for an all-zero tensor).  Entries
    that are exactly zero (check_zero holds the kernel to them exactly) do not count."""
    g = np.abs(ref["g64"][k])
    return None if not g.any() else float((g[g > 0] > bounds(ref, margin)[k]).mean())
