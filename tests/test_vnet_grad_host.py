"""CPU-only: the harness and the case tables of tests/vnet_grad_cases.py on the autograd route (use_kernel=False, a CPU detector)
of OnlineTrainer and meta.meta_train_loop.  The readout 2 * exp_avg is exactly the autograd gradient of that route, g2 = 2 m2 - m1
and the SGD step hold, the route lies inside the bound with the margin 2 (float32 torch on the referee's formulas), and every case
meets the four conditions that make the elementwise check of tests/test_gpu_vnet_grad.py bite: exact zeros (dead ReLU units), the
ReLU margin (asserted inside every referee), at least 99 % of the referee's non-zero entries of dW2 and dW3 above the KERNEL's
bound, and the referee's own gradient with the pass's last sample dropped outside that bound in every tensor."""
import numpy as np
import pytest
import torch

import vnet_grad_cases as G


def test_online_table_is_the_one_stated():
    for S in G.ONLINE_STATES:
        own = [c for c in G.ONLINE.values() if c["S"] == S and c["weights"] == "init"]
        whole = sorted(c["T"] for c in own if c["idx"] is None and not c["env"] and c["labels"] == "word")
        assert whole == sorted(G.WHOLE_T + ((1000,) if S == 16 else ()))
        assert sorted(c["T"] for c in own if c["env"]) == ([33, 49, 136] if S <= 32 else [])
        drawn = [c for c in own if c["name"].startswith(f"S{S}_drawn")]
        assert sorted(c["idx"].shape[1] for c in drawn) == [1, 16, 17, 31, 32, 33, 48, 64] and all(c["T"] == 136 for c in drawn)
        for c in drawn:
            for row in c["idx"].tolist():
                assert len(set(row)) == len(row) and row[0] == 0 and (len(row) == 1 or row[-1] == 135)
        assert G.ONLINE[f"S{S}_dup_T136"]["idx"].tolist() == [[7, 7, 7, 135]]
        perm = G.ONLINE[f"S{S}_perm_T64_M64"]["idx"][0].tolist()
        assert sorted(perm) == list(range(64)) and perm != list(range(64))
        second = sorted((c["T"], 0 if c["idx"] is None else c["idx"].shape[1]) for c in own if c["second"])
        assert second == [(33, 0), (136, 0), (136, 32), (136, 33)]
        assert G.ONLINE[f"S{S}_same_label_T33"]["labels"] == "same"
    g7 = [c for c in G.ONLINE.values() if c["weights"] == "g7"]
    assert len(g7) == 2 + 8 + 1 and all(c["S"] == 16 and c["T"] == 136 for c in g7)
    for c in G.ONLINE.values():
        assert c["idx"] is None or (0 <= int(c["idx"].min()) and int(c["idx"].max()) < c["T"] and c["idx"].shape[0] == 1 + c["second"])


def test_meta_learning_table_is_the_one_stated():
    at16 = [c for c in G.MAML.values() if c["S"] == 16 and not c["env"]]
    assert sorted({c["T"] for c in at16}) == [32, 33, 49, 136] and len(at16) == 17 and sum(c["same"] for c in at16) == 1
    assert len([c for c in G.MAML.values() if c["S"] == 16 and c["env"]]) == 17
    for S in (4, 32, 64, 128):
        own = [(c["T"], c["W"], c["second_order"]) for c in G.MAML.values() if c["S"] == S]
        assert sorted(own) == sorted((T, W, so) for T in (33, 136) for W in (1, 2) for so in (True, False))


@pytest.mark.parametrize("name", G.ONLINE_NAMES)
def test_labels_use_both_ends_of_the_trellis(name):
    case = G.ONLINE[name]
    lab = G.labels_for(case, G.word_of(case))
    S, T = case["S"], case["T"]
    assert lab.dtype == np.int32 and lab.shape == (T,) and lab.min() >= 0 and lab.max() == S - 1
    if case["labels"] == "same":
        assert (lab == S - 1).all()
    elif T > 1:
        assert lab.min() == 0
    if T > G.memory_length(S) and case["labels"] == "word":  # the labels are the word's own trellis states
        tx = torch.from_numpy(G.word_of(case)["bits"].astype(np.float32)).reshape(1, T)
        assert np.array_equal(G.mvn.calculate_states(G.memory_length(S), tx).numpy(), lab)


def _w3_share(case):
    """99 %; G7's saturated softmax: vnet_grad_cases.saturated_share"""
    if case["weights"] != "g7":
        return 0.99
    return G.saturated_share(len(set(case["idx"][0].tolist())) if case["idx"] is not None else case["T"], case["idx"] is None)


@pytest.mark.parametrize("name", G.ONLINE_NAMES)
def test_autograd_route_gradient_per_element(name):
    case = G.ONLINE[name]
    r1, g = G.check_first_iteration(case, "cpu", False, G.MARGIN_AUTOGRAD)
    # the readout is exact: 2 * exp_avg is bitwise the gradient torch.autograd.grad gives this route
    w = G.word_of(case)
    det = G.detector_with(G.weights(case["weights"], case["S"]), case["S"], case["T"], "cpu")
    logits = det(torch.from_numpy(w["y"]).reshape(1, -1), "train").reshape(-1, case["S"])
    lab = torch.from_numpy(G.labels_for(case, w)).long()
    sel = slice(None) if case["idx"] is None else case["idx"][0].long()
    grads = torch.autograd.grad(torch.nn.functional.cross_entropy(logits[sel], lab[sel]), list(det.parameters()))
    for k, (a, b) in enumerate(zip(g, grads)):  # (by value: a dead unit's -0.0 comes back as 0.5 * 0 + 0.5 * -0.0 = +0.0)
        assert np.isfinite(a).all() and np.array_equal(a, b.numpy()), G.NAMES[k]
    samples = case["T"] if case["idx"] is None else case["idx"].shape[1]
    G.check_table_conditions(name, G.reference_of(case), samples, w3_share=_w3_share(case))


@pytest.mark.parametrize("name", G.ONLINE_SECOND_NAMES)
def test_autograd_route_second_iteration(name):
    case = G.ONLINE[name]
    r1 = G.run(case, "cpu", False)
    G.check_second_iteration(case, "cpu", False, G.MARGIN_AUTOGRAD, r1)
    w = G.word_of(case)
    ref2 = G.reference(r1["w"], w["y"], G.labels_for(case, w), None if case["idx"] is None else case["idx"][1])
    G.check_table_conditions(name + " iter 2", ref2, case["T"] if case["idx"] is None else case["idx"].shape[1], w3_share=_w3_share(case))
    # a gradient vector that still holds iteration 1's entries (a first chunk that adds where it must overwrite) is far outside
    stale = G.stale_detection(G.reference_of(case), ref2)
    print(f"{name}: iteration 1's gradient left in g2, in bounds per tensor: {[f'{d:.0f}' for d in stale]}")
    assert stale.min() > 1, (name, stale.tolist())


@pytest.mark.parametrize("S", G.ONLINE_STATES)
def test_permutation_of_all_positions_is_the_whole_word(S):
    """The permuted case poses the whole word's problem: the two cases share one word, every position is drawn once, and their
    float64 referees agree to double rounding (the scale is 1 / 64 both ways).  The kernel meets the samples in the drawn order, so
    its sums over the samples round differently: tests/test_gpu_vnet_grad.py holds the permuted draw to this referee and asks for
    bit identity only of the ascending draw."""
    a, b = G.ONLINE[f"S{S}_perm_T64_M64"], G.ONLINE[f"S{S}_whole_T64"]
    assert G.word_of(a) is G.word_of(b)
    ga, gb = G.reference_of(a)["g64"], G.reference_of(b)["g64"]
    for k in range(6):
        assert np.abs(ga[k] - gb[k]).max() <= 1e-12 * max(np.abs(gb[k]).max(), 1e-300)


@pytest.mark.parametrize("S", G.WORDS_STATES)
def test_autograd_route_train_words(S):
    r1, _ = G.check_words(S, "cpu", False, G.MARGIN_AUTOGRAD)
    ref1, ref2 = G.words_references(S, r1["w"])
    G.check_table_conditions(f"S{S} words", ref1, G.WORDS_M)
    G.check_table_conditions(f"S{S} words iter 2", ref2, G.WORDS_M)
    w = G.train_words_of(S)
    assert w["idx"][:, 0].tolist() == [0, 0] and w["idx"][:, -1].tolist() == [G.WORDS_K - 1] * 2
    assert w["states"].max() == S - 1 and w["states"].min() == 0


@pytest.mark.parametrize("name", [n for n in G.MAML_NAMES if not G.MAML[n]["env"]])
def test_autograd_route_meta_gradient(name):
    """meta.meta_train_loop on the CPU through the same readout; the conditions of the table at theta (support) and theta' (query)."""
    case = G.MAML[name]
    G.check_maml(case, "cpu", False, G.MARGIN_AUTOGRAD)
    G.check_table_conditions("maml " + name, G.maml_reference_of(case), case["T"])
    _, lab, sup, qry = G.maml_inputs(case)
    assert lab[sup].max() == case["S"] - 1 and lab[sup].min() == 0 and lab[qry].max() == case["S"] - 1 and lab[qry].min() == 0
