"""GPU: the gradient of the ViterbiNet training kernels (online_train_kernel, online_train_groups_kernel, online_train_words_kernel,
maml_train_kernel, maml_train_groups_kernel), element by element, against torch autograd in float64 at the shapes where their
loops change form (tests/vnet_grad_cases.py: the readout through Adam's first moment, the case tables, the bound measured from
stock float32 torch and the derivation of the margin of 8; tests/test_vnet_grad_host.py proves on the CPU that the tables bite).

What the tolerance tests of the training kernels cannot see.  test_online_training_vs_torch, ..._at_64_and_128_states_vs_torch,
test_training_kernels_other_state_counts, test_maml_kernel_vs_torch_double_backward and tests/test_gpu_train_words.py run a few
Adam steps and compare weights to |dw| <= 2e-5 + 1e-3 |w| against float32 torch.
  * Adam and RMSprop divide the gradient's scale out: after one step from a zero state the update is lr * sign(g), so a gradient
    with the right signs and the wrong size passes -- 1 / 32 where 1 / M was meant, a chunk counted twice, a sample dropped.
  * Their SGD cases use lr 0.05 to 0.1 for 3 to 5 steps at the same tolerance: one sample dropped from a 136-symbol whole-word
    gradient changes an element by 1 / 136 of itself, which moves a weight by about 1e-3 |g|, below 2e-5 wherever |g| < 2e-2.
  * Every minibatch they draw comes from arange(1, T) or randperm: position 0 and repeated positions never occur; and none
    separates iteration 2's gradient from iteration 1's, although the gradient vector is left as it is after the update (the
    next iteration's first chunk must overwrite it) -- a stale element there is exactly what Adam hides.

tools/vnet_train_gradients.py prints the kernels' error in units of max(d32, floor) per case and tensor
(profiles/vnet_train_gradients.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import vnet_grad_cases as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _all_of(r):
    return r["w"] + r["m"] + r["v"] + [r["loss"]]


@pytest.mark.parametrize("name", G.ONLINE_NAMES)
def test_kernel_gradient_per_element(name):
    """|g - g64| <= 8 max(d32, floor) for every element of the six tensors, exact zeros where the referee has them, the loss,
    exp_avg_sq to 4 ulp and the SGD step to 1 ulp; the kernel that ran is the one the case is about (vnet_grad_cases.run).
    S16_drawn_T136_M1_g7 (one decided sample under G7's trained weights) is the case that found the kernels' softmax rounding lse =
    max + logf(sum) at the size of the largest logit: 19 ... 26 units in all six tensors before they took torch's order
    (x - max) - logf(sum); vnet_grad_cases' docstring has the arithmetic, profiles/vnet_train_gradients.txt the measured table."""
    G.check_first_iteration(G.ONLINE[name], DEV, True, G.MARGIN_KERNEL)


@pytest.mark.parametrize("name", G.ONLINE_SECOND_NAMES)
def test_kernel_second_iteration_gradient(name):
    """After a step that moved every weight with a gradient by 0.02: the gradient of iteration 2 alone, at the kernel's own weights
    (a first chunk that adds to the gradient vector where it must overwrite it is off by all of iteration 1's gradient)."""
    G.check_second_iteration(G.ONLINE[name], DEV, True, G.MARGIN_KERNEL)


@pytest.mark.parametrize("S", G.ONLINE_STATES)
def test_permutation_of_all_positions_is_the_whole_word(S):
    """M = 64 distinct positions of T = 64: every count is 1 and the scale 1 / 64 both ways, but the samples meet the chunks in
    another order, so the sums over the samples round differently: the whole word to the bound (both are held to the referee
    above), and bit for bit once the drawn positions are in ascending order."""
    perm, whole = G.ONLINE[f"S{S}_perm_T64_M64"], G.ONLINE[f"S{S}_whole_T64"]
    ascending = dict(perm, idx=torch.arange(64, dtype=torch.int32).reshape(1, 64))
    a, b = G.run(ascending, DEV, True), G.run(whole, DEV, True)
    assert _bits_equal(_all_of(a), _all_of(b))
    g, ref = G.readout(G.run(perm, DEV, True)), G.reference_of(whole)
    G.compare(perm["name"] + " against the whole word's referee", g, ref, G.MARGIN_KERNEL)


@pytest.mark.parametrize("S", [S for S in G.ONLINE_STATES if S <= 32])
@pytest.mark.parametrize("T", [33, 49, 136])
def test_one_workgroup_per_chunk_equals_one_workgroup(S, T):
    """online_train_groups_kernel and online_train_kernel on the same whole word: both are read against the referee above, and
    they agree bit for bit (the gradient slots are added in chunk order)."""
    a = G.run(G.ONLINE[f"S{S}_whole_T{T}"], DEV, True)
    b = G.run(G.ONLINE[f"S{S}_whole_T{T}_groups0"], DEV, True)
    assert _bits_equal(_all_of(a), _all_of(b))


@pytest.mark.parametrize("S", G.WORDS_STATES)
def test_train_words_gradient_and_raw_abi(S):
    """online_train_words_kernel<SC>: two words, word_of_iter = [1, 0], K = 120 < T = 136, M = 33 -- the gradient of iteration 1
    alone and of iteration 2 against the referee; then mvn_vnet_train_words_f32 itself on padded rows (y_ld = T + 5 with NaN behind
    the word, labels_ld = K + 3 with the out-of-range state S + 7 behind the labels): bit-identical to the trainer's call."""
    _, r2 = G.check_words(S, DEV, True, G.MARGIN_KERNEL)
    w, T, K, M = G.train_words_of(S), G.WORDS_T, G.WORDS_K, G.WORDS_M
    y_ld, lab_ld = T + 5, K + 3
    y_pad = np.full((2, y_ld), np.nan, np.float32)
    y_pad[:, :T] = w["y"]
    lab_pad = np.full((2, lab_ld), S + 7, np.int32)
    lab_pad[:, :K] = w["states"]
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    y_d, lab_d = torch.from_numpy(y_pad).to(DEV), torch.from_numpy(lab_pad).to(DEV)
    woi = torch.tensor(G.WORD_OF_ITER, dtype=torch.int32, device=DEV)
    idx_d = torch.from_numpy(w["idx"]).to(DEV).contiguous()
    p = [torch.from_numpy(a.copy()).to(DEV) for a in G.weights("init", S)]
    P = int(G.offsets(S)[-1])
    m, v = torch.zeros(P, device=DEV), torch.zeros(P, device=DEV)
    loss_d = torch.full((2,), float("nan"), device=DEV)
    with mvn._lib.on_device(DEV):
        rc = lib.mvn_vnet_train_words_f32(ptr(y_d), y_ld, ptr(lab_d), lab_ld, 2, K, ptr(woi), ptr(idx_d), M, 2, *[ptr(t) for t in p],
                                          ptr(m), ptr(v), 0, G.LR, G.BETAS[0], G.BETAS[1], 1e-8, ptr(loss_d), S,
                                          mvn._lib.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in p] + G.split(m, S) + G.split(v, S) + [loss_d.cpu().numpy()]
    assert all(np.isfinite(a).all() for a in got)
    assert _bits_equal(got, _all_of(r2))


@pytest.mark.parametrize("name", G.MAML_NAMES)
def test_kernel_meta_gradient_per_element(name):
    """One meta-learning step from a zero state: exp_avg holds half the meta-gradient -- every element within 8 max(d32, floor) of
    the float64 double backward (second order) or of the query gradient at theta' (first order), exact zeros, the query loss."""
    G.check_maml(G.MAML[name], DEV, True, G.MARGIN_KERNEL)


@pytest.mark.parametrize("name", [n for n in G.MAML_NAMES if G.MAML[n]["env"]])
def test_meta_learning_groups_equal_one_workgroup(name):
    a = G.run_maml(G.MAML[name.replace("_groups0", "")], DEV, True)
    b = G.run_maml(G.MAML[name], DEV, True)
    assert _bits_equal(_all_of(a), _all_of(b))


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("name", ["drawn_T136_M33", "whole_T49"])
def test_trial_batched_form_at_64_and_128_states_is_the_single_trial_kernel(S, name):
    """online_train_kernel<64 | 128, true> through mvn_vnet_online_train_trials_f32 (three trials, the middle one inactive): two
    iterations of the case, bit-identical to online_train_kernel<64 | 128, false> -- the one trial-batched form no other test pins
    to its single-trial twin bit for bit (vnet_grad_cases' docstring lists the tests that pin the others)."""
    from meta_viterbinet_amd import trials as tr_mod

    case = G.ONLINE[f"S{S}_{name}"]
    T, n, R = case["T"], 2, 3
    idx = case["idx"]
    if idx is not None and idx.shape[0] < n:
        idx = torch.from_numpy(G.draw(T, idx.shape[1], n, 64 + S))
    case = dict(case, idx=idx)
    want = G.run(case, DEV, True, n=n)
    w = G.word_of(case)
    y = torch.from_numpy(w["y"]).to(DEV)
    lab = torch.from_numpy(G.labels_for(case, w)).to(DEV)
    idx_d = None if idx is None else idx.to(DEV).contiguous()
    M = 0 if idx is None else idx.shape[1]
    P = int(G.offsets(S)[-1])
    ws = [[torch.from_numpy(a.copy()).to(DEV) for a in G.weights(case["weights"], S)] for _ in range(R)]
    m, v = torch.zeros(R, P, device=DEV), torch.zeros(R, P, device=DEV)
    loss = torch.full((R, n), float("nan"), device=DEV)
    status = torch.zeros(R, dtype=torch.int32, device=DEV)
    d = np.zeros(R, dtype=tr_mod.TRIAL_DTYPE)
    for r in range(R):
        d[r]["y"], d[r]["labels"], d[r]["idx"] = y.data_ptr(), lab.data_ptr(), 0 if idx_d is None else idx_d.data_ptr()
        d[r]["w_in"] = d[r]["w_out"] = [t.data_ptr() for t in ws[r]]
        d[r]["adam_m"], d[r]["adam_v"], d[r]["loss_out"] = m[r].data_ptr(), v[r].data_ptr(), loss[r].data_ptr()
        d[r]["status"] = status[r:].data_ptr()
        d[r]["b1pow"], d[r]["b2pow"] = 1.0, 1.0
        d[r]["n"] = 0 if r == 1 else n
    dd = torch.from_numpy(d.view(np.uint8)).to(DEV)
    lib = mvn._lib.load()
    named = ctypes.create_string_buffer(128)
    assert lib.mvn_vnet_train_kernel_name(0, R, T, M, S, 0, named, 128) == 0
    assert named.value.decode() == f"online_train_kernel<{S}, true> 1x{R}", named.value
    with mvn._lib.on_device(DEV):
        rc = lib.mvn_vnet_online_train_trials_f32(mvn._lib.ptr(dd), R, T, M, G.LR, G.BETAS[0], G.BETAS[1], 1e-8, S, None, 0,
                                                  mvn._lib.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    assert not m[1].any() and all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(ws[1], G.weights(case["weights"], S)))
    for r in (0, 2):
        got = [t.cpu().numpy() for t in ws[r]] + G.split(m[r], S) + G.split(v[r], S) + [loss[r].cpu().numpy()]
        assert _bits_equal(got, _all_of(want)), r
