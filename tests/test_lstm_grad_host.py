"""CPU-only: the harness and the case table of tests/lstm_grad_cases.py on the autograd route (use_kernel=False, the CPU route) of
LSTMOnlineTrainer.  The readout 2 * exp_avg is bitwise the autograd gradient of that route; the route lies inside the bound with
the margin 2 (float32 torch on the referee's formulas); and in every case at least 99 % of the referee's entries of W_ih1, W_hh1
and fc_W exceed the KERNEL's bound in magnitude, so the elementwise check of tests/test_gpu_lstm_grad.py is not vacuous."""
import numpy as np
import pytest
import torch

import lstm_grad_cases as G
from meta_viterbinet_amd import lstm as L
from test_lstm_train_host import detector_with


def test_case_table_is_the_one_stated():
    forms = {"whole": 0, "one": 0, "dup": 0, "drawn": 0, "perm": 0}
    for n in G.CASE_NAMES:
        if not n.endswith("_g18"):
            forms[n.split("_")[0]] += 1
    assert forms == {"whole": 9, "one": 3, "dup": 3, "drawn": 3, "perm": 1}
    assert sorted(G.CASES[n]["T"] for n in G.CASE_NAMES if n.startswith("whole") and not n.endswith("g18")) == [1, 2, 3, 4, 5, 40, 136, 255, 256]
    assert [n for n in G.CASE_NAMES if n.endswith("_g18")] == ["whole_T136_g18", "dup_T136_g18", "drawn_T136_M32_g18"]
    assert sorted(G.CASES[n]["T"] for n in G.SECOND_NAMES) == [2, 136, 136, 256]
    perm = G.CASES["perm_T256_M256"]["idx"]
    assert sorted(perm[0].tolist()) == list(range(256)) and perm[0].tolist() != list(range(256))
    for n in G.DUPLICATE_NAMES:
        row = G.CASES[n]["idx"][0].tolist()
        assert len(set(row)) < len(row)
    for n in ("drawn_T136_M32", "drawn_T40_M32"):
        assert all(len(set(r.tolist())) == 32 for r in G.CASES[n]["idx"])
    for c in G.CASES.values():
        assert c["idx"] is None or (0 <= int(c["idx"].min()) and int(c["idx"].max()) < c["T"] and c["idx"].shape[0] == 1 + c["second"])


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_autograd_route_gradient_per_element(name):
    case = G.CASES[name]
    r1, g = G.check_first_iteration(case, "cpu", False, G.MARGIN_AUTOGRAD)
    # the readout is exact: 2 * exp_avg is bitwise the gradient torch.autograd.grad gives this route
    bits, rx = G.word(case["T"])
    det = detector_with(G.weights(case["weights"]))
    logits = det(torch.from_numpy(rx), "train").reshape(-1, L.N_CLASSES)
    lab = torch.from_numpy(bits).long()[0]
    sel = slice(None) if case["idx"] is None else case["idx"][0].long()
    grads = torch.autograd.grad(torch.nn.functional.cross_entropy(logits[sel], lab[sel]), det._params())
    for k, (a, b) in enumerate(zip(g, grads)):
        assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32)), G.NAMES[k]
    # not vacuous: the share of the referee's entries above the bound the kernel is held to
    ref = G.reference_of(case)
    for k in G.SHARE_TENSORS:
        share = G.share_above_bound(ref, G.MARGIN_KERNEL, k)
        print(f"{name}: {G.NAMES[k]}: share of |g64| above the kernel's bound: {share}")
        assert share is None or share >= 0.99, (name, G.NAMES[k], share)
        assert share is not None or k in case["zero"]


@pytest.mark.parametrize("name", G.SECOND_NAMES)
def test_autograd_route_second_iteration(name):
    G.check_second_iteration(G.CASES[name], "cpu", False, G.MARGIN_AUTOGRAD)
