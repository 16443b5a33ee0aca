"""CPU-only twin of tests/test_gpu_vnet_grad_256.py: the 256-state table of tests/vnet_grad_cases_256.py on the autograd route
(use_kernel=False, a CPU detector), held to the margin 2, and the conditions that make the kernel's elementwise check bite at this
state count -- exact zeros, the ReLU margin (asserted inside every referee), at least 99 % of the referee's non-zero dW2 and dW3
above the KERNEL's bound, a dropped sample outside it in every tensor, and, for every second-iteration case, iteration 1's gradient
left in g2 outside it: what a first chunk that ADDS to dW3's accumulators where it must overwrite them would leave."""
import numpy as np
import pytest

import vnet_grad_cases as G
import vnet_grad_cases_256 as C


@pytest.fixture(scope="module", autouse=True)
def _words():
    C.words()


def test_table_is_the_one_stated():
    own = list(C.CASES.values())
    assert all(c["S"] == 256 and c["weights"] == "init" and not c["env"] for c in own)
    assert sorted(c["T"] for c in own if c["idx"] is None and c["labels"] == "word") == sorted(G.WHOLE_T)
    drawn = [c for c in own if c["name"].startswith("S256_drawn")]
    assert sorted(c["idx"].shape[1] for c in drawn) == sorted(G.MINIBATCH_M) and all(c["T"] == 136 for c in drawn)
    for c in drawn:
        for row in c["idx"].tolist():
            assert len(set(row)) == len(row) and row[0] == 0 and (len(row) == 1 or row[-1] == 135)
    assert C.CASES["S256_dup_T136"]["idx"].tolist() == [[7, 7, 7, 135]]
    perm = C.CASES["S256_perm_T64_M64"]["idx"][0].tolist()
    assert sorted(perm) == list(range(64)) and perm != list(range(64))
    assert sorted((c["T"], 0 if c["idx"] is None else c["idx"].shape[1]) for c in own if c["second"]) == [(33, 0), (136, 0), (136, 32), (136, 33)]
    assert C.CASES["S256_same_label_T33"]["labels"] == "same"
    for c in own:
        assert c["idx"] is None or (0 <= int(c["idx"].min()) and int(c["idx"].max()) < c["T"] and c["idx"].shape[0] == 1 + c["second"])
        lab = G.labels_for(c, G.word_of(c))
        assert lab.max() == 255 and (c["labels"] == "same" or c["T"] == 1 or lab.min() == 0)


@pytest.mark.parametrize("name", C.NAMES)
def test_autograd_route_gradient_per_element(name):
    case = C.CASES[name]
    G.check_first_iteration(case, "cpu", False, G.MARGIN_AUTOGRAD)
    G.check_table_conditions(name, G.reference_of(case), C.samples_of(case))


@pytest.mark.parametrize("name", C.SECOND_NAMES)
def test_autograd_route_second_iteration(name):
    case = C.CASES[name]
    r1 = G.run(case, "cpu", False)
    G.check_second_iteration(case, "cpu", False, G.MARGIN_AUTOGRAD, r1)
    w = G.word_of(case)
    ref2 = G.reference(r1["w"], w["y"], G.labels_for(case, w), None if case["idx"] is None else case["idx"][1])
    G.check_table_conditions(name + " iter 2", ref2, C.samples_of(case))
    stale = G.stale_detection(G.reference_of(case), ref2)
    print(f"{name}: iteration 1's gradient left in g2, in bounds per tensor: {[f'{d:.0f}' for d in stale]}")
    assert stale.min() > 1, (name, stale.tolist())


def test_permutation_of_all_positions_is_the_whole_word():
    a, b = C.CASES["S256_perm_T64_M64"], C.CASES["S256_whole_T64"]
    assert G.word_of(a) is G.word_of(b)
    ga, gb = G.reference_of(a)["g64"], G.reference_of(b)["g64"]
    for k in range(6):
        assert np.abs(ga[k] - gb[k]).max() <= 1e-12 * max(np.abs(gb[k]).max(), 1e-300)


def test_autograd_route_train_words():
    r1, _ = G.check_words(256, "cpu", False, G.MARGIN_AUTOGRAD)
    ref1, ref2 = G.words_references(256, r1["w"])
    G.check_table_conditions("S256 words", ref1, G.WORDS_M)
    G.check_table_conditions("S256 words iter 2", ref2, G.WORDS_M)
    stale = G.stale_detection(ref1, ref2)
    assert stale.min() > 1, stale.tolist()
    w = G.train_words_of(256)
    # (state 0 -- eight zeros in a row -- sits at position 135 of the drawn words, behind the K = 120 labelled positions)
    assert w["states"].max() == 255 and w["states"].min() < 16 and len(np.unique(w["states"])) > 100
