"""The meta-learning kernel at 64 and 128 states (maml_train_kernel<64 | 128, false>: two parameter vectors in LDS, theta waiting in
the weight arrays during the query pass, the Hessian pass in 16-sample chunks with H v in registers) against meta.meta_train_loop =
torch autograd with create_graph on the same device, and the recorded runs of the unmodified reference as METAVNETTrainer at
channel memories 6 and 7 (golden G21, tests/golden/make_golden_meta_states.py).

Tolerances are those of the kernel's test at <= 32 states (test_gpu_parity.test_maml_kernel_vs_torch_double_backward):
|dw| <= 2e-5 + 1e-3 |w|, query loss rtol 2e-4 atol 1e-6, exp_avg rtol 1e-3 atol 1e-6.  Weights: G17's starting weights (the
reference's own trainer produced them); received words: G21's rx rows; labels: random bits through calculate_states.  That the
second-order term matters at these inputs is asserted on the CPU in float64 (second_order_share): a missing or wrong H v cannot
hide inside the tolerances."""
import functools

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import test_gpu_reference_flow as RF

pytestmark = pytest.mark.gpu

STATES = {64: 6, 128: 7}  # n_states: channel memory
META_LR = 0.1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _vnet_with(w, S, T, dev):
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w):
            p.copy_(torch.as_tensor(a))
    return det


@functools.lru_cache(maxsize=None)
def _inputs(S, T):
    """(weights, rx [10, T], tx [10, T], labels [10, T]) on the CPU, the same arrays for every test that asks"""
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g17, g21 = np.load(os.path.join(here, "g17_by_word_64_128_states.npz")), np.load(os.path.join(here, "g21_by_word_meta_64_128_states.npz"))
    L = STATES[S]
    w = [g17[f"L{L}_selfsup_w0_{i}"] for i in range(6)]
    assert w[4].shape == (S, 50)
    rx = np.ascontiguousarray(g21[f"L{L}_meta_rx"][:10, :T]).astype(np.float32)
    tx = np.random.RandomState(100 + S).randint(0, 2, (10, T)).astype(np.float32)
    labels = mvn.calculate_states(L, torch.tensor(tx)).reshape(10, T).numpy()
    assert labels.min() >= 0 and labels.max() < S and labels.max() >= S // 2 and (labels >= S // 2).sum() >= T  # the upper half too
    return w, rx, tx, labels


def _meta_grad64(w, rx, labels, sup, qry, MAML):
    """the meta-gradient of one step in float64 on the CPU (plain autograd on the network written out)"""
    p = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in w]

    def loss(params, words):
        y = torch.tensor(rx[words].reshape(-1, 1).astype(np.float64))
        lab = torch.tensor(labels[words].reshape(-1).astype(np.int64))
        h1 = torch.sigmoid(y @ params[0].T + params[1])
        a2 = torch.relu(h1 @ params[2].T + params[3])
        return torch.nn.functional.cross_entropy(a2 @ params[4].T + params[5], lab)

    gs = torch.autograd.grad(loss(p, sup), p, create_graph=MAML)
    upd = [a - META_LR * g for a, g in zip(p, gs)]
    return [g.numpy() for g in torch.autograd.grad(loss(upd, [qry]), p)]


@functools.lru_cache(maxsize=None)
def second_order_share(S, W):
    """per parameter array: max |second-order term| / max |meta-gradient| in float64, for the step (support words 1 .. W, query W + 1)"""
    w, rx, _, labels = _inputs(S, 136)
    sup, qry = list(range(1, 1 + W)), 1 + W
    full, first = _meta_grad64(w, rx, labels, sup, qry, True), _meta_grad64(w, rx, labels, sup, qry, False)
    return [float(np.abs(a - b).max() / np.abs(a).max()) for a, b in zip(full, first)]


def _steps(n_steps, W, dev):
    sup = torch.stack([torch.arange(k - W, k, device=dev) for k in range(n_steps)])  # step 0 uses negative indices
    return sup, torch.arange(n_steps, device=dev)


def _pair(S, T, dev, seeded):
    """two detectors with their trainers in the same state, and the words on the device"""
    w, rx, tx, _ = _inputs(S, T)
    dets = [_vnet_with(w, S, T, dev) for _ in range(2)]
    trs = [mvn.OnlineTrainer(d, STATES[S]) for d in dets]
    if seeded:
        gen = torch.Generator(device=dev).manual_seed(5 + S)
        trs[0].exp_avg.normal_(0, 1e-3, generator=gen)
        trs[0].exp_avg_sq.uniform_(1e-7, 1e-5, generator=gen)
        trs[1].exp_avg.copy_(trs[0].exp_avg)
        trs[1].exp_avg_sq.copy_(trs[0].exp_avg_sq)
        for tr in trs:
            tr.step = 4
    return dets, trs, torch.tensor(rx, device=dev), torch.tensor(tx, device=dev)


def _against_autograd(S, T, W, MAML, n_steps, calls, dev):
    dets, trs, rxw, txw = _pair(S, T, dev, True)
    meta = mvn.META_VNETDetector(S, {"train": T, "val": T})
    sup, qry = _steps(n_steps, W, dev)
    ref_loss = [float(mvn.meta_train_loop(dets[0], meta, trs[0], rxw, txw, sup[k], qry[k:k + 1], META_LR, MAML)) for k in range(n_steps)]
    loss, at = [], 0
    for n in calls:
        loss.append(trs[1].maml_training(rxw, txw, sup[at:at + n], qry[at:at + n], META_LR, MAML, return_loss=True))
        at += n
    assert at == n_steps and trs[1].step == trs[0].step == 4 + n_steps
    loss = _np(torch.cat(loss))
    dw = max(float((torch.abs(a - b) / (2e-5 + 1e-3 * torch.abs(b))).max().detach())
             for a, b in zip(dets[1].parameters(), dets[0].parameters()))
    print(f"S={S} T={T} W={W} MAML={MAML}: {n_steps} steps, query loss {ref_loss[0]:.4f} -> {ref_loss[-1]:.4f}, worst |loss - torch's| "
          f"{np.abs(loss - np.array(ref_loss)).max():.2e}, worst |dw| / tolerance {dw:.3f}")
    assert np.all(np.isfinite(loss))
    assert np.allclose(loss, np.array(ref_loss), rtol=2e-4, atol=1e-6)
    for a, b in zip(dets[1].parameters(), dets[0].parameters()):
        assert bool((torch.abs(a - b) <= 2e-5 + 1e-3 * torch.abs(b)).all())
    assert torch.allclose(trs[1].exp_avg, trs[0].exp_avg, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("MAML", [True, False], ids=["second_order", "first_order"])
@pytest.mark.parametrize("S", [64, 128])
def test_steps_against_autograd(dev, S, MAML, W):
    """Six steps on words of 136 symbols as two calls (4 + 2: the Adam state and the weights carry over), moments pre-seeded, step 0
    with negative support indices."""
    share = second_order_share(S, W)
    print(f"S={S} W={W}: second-order term / largest meta-gradient entry per array (float64): {[round(s, 3) for s in share]}")
    assert min(share) >= 0.05
    _against_autograd(S, 136, W, MAML, 6, (4, 2), dev)


@pytest.mark.parametrize("T,W", [(16, 1), (24, 2), (33, 1), (40, 1)])
@pytest.mark.parametrize("S", [64, 128])
def test_smallest_shapes(dev, S, T, W):
    """(16, 1): one chunk that is both a pass's first and <= 16 samples; (24, 2): 48 support samples, the word boundary inside a
    gradient chunk and inside a 16-row Hessian chunk; (33, 1): 32 + 1; (40, 1): 32 + a tail of 8 in the gradient passes,
    16 + 16 + 8 in the Hessian pass."""
    _against_autograd(S, T, W, True, 3, (3,), dev)


@pytest.mark.parametrize("MAML", [True, False], ids=["second_order", "first_order"])
@pytest.mark.parametrize("S", [64, 128])
def test_meta_gradient_per_element(dev, S, MAML):
    """One step from zero moments and step 0: exp_avg = 0.1 x the meta-gradient, every element against autograd's at the exp_avg
    tolerance.  An element outside it is taken to the float64 run of the same step (test_gpu_replay's referee rule): the kernel may
    be twice as far from float64 as torch's fp32 is, plus one tolerance.
    Measured (MI355X), largest |x - float64| per array W1 b1 W2 b2 W3 b3 in units of 0.1 x the array's largest meta-gradient entry:
    see DESIGN 5.5; every element was inside the plain tolerance."""
    T, W = 136, 1
    dets, trs, rxw, txw = _pair(S, T, dev, False)
    w, rx, _, labels = _inputs(S, T)
    meta = mvn.META_VNETDetector(S, {"train": T, "val": T})
    sup, qry = torch.tensor([[1]], device=dev), torch.tensor([2], device=dev)
    mvn.meta_train_loop(dets[0], meta, trs[0], rxw, txw, sup[0], qry, META_LR, MAML)
    trs[1].maml_training(rxw, txw, sup, qry, META_LR, MAML)
    g64 = _meta_grad64(w, rx, labels, [1], 2, MAML)
    k, t = _np(trs[1].exp_avg).astype(np.float64), _np(trs[0].exp_avg).astype(np.float64)
    f = 0.1 * np.concatenate([a.reshape(-1) for a in g64])
    tol = 1e-6 + 1e-3 * np.abs(t)
    outside = np.abs(k - t) > tol
    at, dev_k, dev_t = 0, [], []
    for a in g64:
        sl = slice(at, at + a.size)
        scale = np.abs(f[sl]).max()
        dev_k.append(float(np.abs(k[sl] - f[sl]).max() / scale))
        dev_t.append(float(np.abs(t[sl] - f[sl]).max() / scale))
        at += a.size
    ratio = float((np.abs(k - f) / (2.0 * np.abs(t - f) + tol)).max())
    print(f"S={S} MAML={MAML}: largest |x - float64| per array relative to the array's largest entry: kernel {['%.1e' % v for v in dev_k]}, "
          f"torch fp32 {['%.1e' % v for v in dev_t]}; {int(outside.sum())} of {k.size} elements outside the plain tolerance; "
          f"referee ratio |kernel - f64| / (2 |torch - f64| + tol) worst {ratio:.3f}")
    assert np.abs(f).max() > 1e-4  # (a real gradient)
    assert np.all(~outside | (np.abs(k - f) <= 2.0 * np.abs(t - f) + tol))


@pytest.mark.parametrize("S", [64, 128])
def test_determinism_and_state(dev, S):
    T = 136
    w, rx, tx, _ = _inputs(S, T)
    rxw, txw = torch.tensor(rx, device=dev), torch.tensor(tx, device=dev)
    sup, qry = _steps(3, 1, dev)

    def run(meta_lr, MAML):
        det = _vnet_with(w, S, T, dev)
        tr = mvn.OnlineTrainer(det, STATES[S])
        loss = tr.maml_training(rxw, txw, sup, qry, meta_lr, MAML, return_loss=True)
        return [p.detach().clone() for p in det.parameters()] + [tr.exp_avg.clone(), tr.exp_avg_sq.clone(), loss]

    for MAML in (True, False):
        a, b = run(META_LR, MAML), run(META_LR, MAML)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), MAML
    zero, first = run(0.0, False), run(META_LR, False)
    assert all(bool(torch.isfinite(x).all()) for x in zero)
    assert not torch.equal(zero[4], first[4]) and not torch.equal(zero[-1], first[-1])  # the inner step is not a no-op
    for x, y in zip(zero[:6], [torch.as_tensor(a) for a in w]):
        assert not torch.equal(x.cpu(), y)  # theta came back from where it waited and took its Adam steps


# ---- golden G21: the reference's METAVNETTrainer runs at 64 and 128 states
def _flow(golden, tag, dev, hip, blocks=None, **more):
    """test_gpu_reference_flow._run for a G21 flow (G16's `meta` settings; FLOWS there has no key for it)"""
    g = golden("g21_by_word_meta_64_128_states")
    ss_it, meta_it, j_num, meta_sub, _, subframes, nsym = [int(v) for v in g[f"{tag}_meta"]]
    tx = torch.tensor(g[f"{tag}_tx"][:blocks], device=dev).float()
    rx = torch.tensor(g[f"{tag}_rx"][:blocks], device=dev)
    T = rx.shape[1]
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    S = w0[5].shape[0]
    det = _vnet_with(w0, S, T, dev)
    tr = mvn.OnlineTrainer(det, STATES[S], use_kernel=hip)
    draws = RF._recorded(g, tag, dev)
    last = {}

    def observer(seen):
        if seen["stage"] == "end" and seen["saved_detector"] is not None:
            last["saved"] = [_np(p).copy() for p in seen["saved_detector"].parameters()]

    kw = dict(self_supervised=True, self_supervised_iterations=ss_it, ser_thresh=0.02, online_meta=True, meta_lr=0.1, MAML=True,
              window_size=1, meta_train_iterations=meta_it, meta_j_num=j_num, meta_subframes=meta_sub, meta_style_online_training=True,
              meta_detector=mvn.META_VNETDetector(S, {"train": T, "val": T}), online_trainer=tr, draws=draws, observer=observer)
    kw.update(more)
    ser = mvn.eval_by_word(det, tx, rx, 9.0, 0.2, nsym, subframes, **kw)
    return g, ser, draws, [_np(p) for p in det.parameters()], last.get("saved")


def test_route(golden, dev, monkeypatch):
    """eval_by_word with online_meta at 64 states takes the meta-learning kernel by default and builds no graphed step; with
    hip_meta=False it is the other way round; both report the same ser_by_word (the first 16 blocks of G21's L6_meta: three updates)."""
    from meta_viterbinet_amd import meta as meta_mod

    calls = {"kernel": 0, "graph": 0}
    real_maml, real_init = mvn.OnlineTrainer.maml_training, meta_mod.GraphedMetaStep.__init__

    def maml_spy(self, *a, **k):
        calls["kernel"] += 1
        return real_maml(self, *a, **k)

    def init_spy(self, *a, **k):
        calls["graph"] += 1
        return real_init(self, *a, **k)

    monkeypatch.setattr(mvn.OnlineTrainer, "maml_training", maml_spy)
    monkeypatch.setattr(meta_mod.GraphedMetaStep, "__init__", init_spy)
    g, ser_k, _, _, _ = _flow(golden, "L6_meta", dev, True, blocks=16)
    assert calls == {"kernel": 3, "graph": 0}, calls
    _, ser_g, _, _, _ = _flow(golden, "L6_meta", dev, True, blocks=16, hip_meta=False)
    assert calls == {"kernel": 3, "graph": 1}, calls
    assert np.array_equal(ser_k, ser_g) and np.array_equal(ser_k, g["L6_meta_ser_by_word"][:16])


@pytest.mark.parametrize("route", ["hip_kernels", "torch_autograd"])
@pytest.mark.parametrize("tag", ["L6_meta", "L7_meta"])
def test_reference_meta_flow_64_128_states(golden, dev, tag, route):
    """Golden G21 like test_reference_by_word_flow_other_state_counts: ser_by_word identical to the reference's on all 50 blocks,
    every recorded draw used, final and saved weights within 5e-5 of the reference's."""
    hip = route == "hip_kernels"
    g, ser, draws, w, saved = _flow(golden, tag, dev, hip, hip_meta=hip, graphed_meta=False)
    ref = g[f"{tag}_ser_by_word"]
    assert ser.shape == ref.shape == (50,)
    assert np.array_equal(ser, ref), (np.flatnonzero(ser != ref), ser[ser != ref], ref[ser != ref])
    assert draws.used_up(), (draws.r_at, len(draws.randint))
    moved = max(float(np.abs(g[f"{tag}_w1_{i}"] - g[f"{tag}_w0_{i}"]).max()) for i in range(6))
    worst = max(float(np.abs(w[i] - g[f"{tag}_w1_{i}"]).max()) for i in range(6))
    worst_s = max(float(np.abs(saved[i] - g[f"{tag}_saved_{i}"]).max()) for i in range(6))
    print(f"g21 {tag} {route}: ser identical on 50 blocks ({int((ref > 0).sum())} with bit errors); weights moved {moved:.4f}, end "
          f"{worst:.2e} from the reference's, saved weights {worst_s:.2e}")
    assert moved > 0.005 and worst <= 5e-5 and worst_s <= 5e-5
