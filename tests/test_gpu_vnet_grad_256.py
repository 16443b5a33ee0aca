"""GPU: the gradient of the 256-state training kernels -- online_train_kernel<256, false> and the word axis'
online_train_words_states256_kernel -- element by element against torch autograd in float64, with tests/vnet_grad_cases.py's
readout, referee, bound and margin of 8 on the table of tests/vnet_grad_cases_256.py (tests/test_vnet_grad_256_host.py proves on
the CPU that the table bites).

What is new at this state count: W3's gradient does not fit the LDS beside the parameters, so it stays in the MFMA accumulators
that compute it, four 16 x 16 tiles per wave, across the chunks of a pass, and meets the optimizer there.  The first chunk of a pass
must OVERWRITE those registers and every further one add to them -- 16- and 32-row chunks alike -- which is what the whole-word
lengths around the chunk sizes and the second-iteration cases pin (iteration 1's gradient left in iteration 2's is hundreds of
bounds off); db3 moved inside the gradient vector (it follows db2), and the 32 logits tiles go two to a wave.
vnet_grad_cases.run asserts through mvn_vnet_train_kernel_name that the 256-state kernel is what runs."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import vnet_grad_cases as G
import vnet_grad_cases_256 as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 256


@pytest.fixture(scope="module", autouse=True)
def _words():
    C.words()


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _all_of(r):
    return r["w"] + r["m"] + r["v"] + [r["loss"]]


@pytest.mark.parametrize("name", C.NAMES)
def test_kernel_gradient_per_element(name):
    """|g - g64| <= 8 max(d32, floor) for every element of the six tensors, exact zeros where the referee has them, the loss,
    exp_avg_sq to 4 ulp and one SGD step with lr = 64 to 1 ulp."""
    case = C.CASES[name]
    assert G.expected_online_kernel(case) == "online_train_kernel<256, false> 1x1"
    G.check_first_iteration(case, DEV, True, G.MARGIN_KERNEL)


@pytest.mark.parametrize("name", C.SECOND_NAMES)
def test_kernel_second_iteration_gradient(name):
    """The gradient of iteration 2 alone, at the kernel's own weights after a step that moved every weight with a gradient by 0.02."""
    G.check_second_iteration(C.CASES[name], DEV, True, G.MARGIN_KERNEL)


def test_permutation_of_all_positions_is_the_whole_word():
    """M = 64 distinct positions of T = 64 in another order: the whole word's referee to the bound, and bit for bit the whole word
    once the drawn positions are in ascending order."""
    perm, whole = C.CASES["S256_perm_T64_M64"], C.CASES["S256_whole_T64"]
    ascending = dict(perm, idx=torch.arange(64, dtype=torch.int32).reshape(1, 64))
    a, b = G.run(ascending, DEV, True), G.run(whole, DEV, True)
    assert _bits_equal(_all_of(a), _all_of(b))
    g, ref = G.readout(G.run(perm, DEV, True)), G.reference_of(whole)
    G.compare(perm["name"] + " against the whole word's referee", g, ref, G.MARGIN_KERNEL)


def test_same_inputs_give_the_same_bits():
    """Two iterations of a two-chunk minibatch and of the whole word, run twice: every weight, moment and loss bit for bit."""
    for name in ("S256_drawn_T136_M33", "S256_whole_T136"):
        a, b = G.run(C.CASES[name], DEV, True, n=2), G.run(C.CASES[name], DEV, True, n=2)
        assert _bits_equal(_all_of(a), _all_of(b)), name


def test_train_words_gradient_and_raw_abi():
    """online_train_words_states256_kernel: two words, word_of_iter = [1, 0], K = 120 < T = 136, M = 33 -- the gradient of
    iteration 1 alone and of iteration 2 against the referee; then mvn_vnet_train_words_states_f32 itself on padded rows (y_ld = T + 5
    with NaN behind the word, labels_ld = K + 3 with the out-of-range state S + 7 behind the labels): bit-identical to the trainer's call."""
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
        rc = lib.mvn_vnet_train_words_states_f32(ptr(y_d), y_ld, ptr(lab_d), lab_ld, 2, K, ptr(woi), ptr(idx_d), M, 2, *[ptr(t) for t in p],
                                                 ptr(m), ptr(v), 0, G.LR, G.BETAS[0], G.BETAS[1], 1e-8, ptr(loss_d), S,
                                                 mvn._lib.current_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in p] + G.split(m, S) + G.split(v, S) + [loss_d.cpu().numpy()]
    assert all(np.isfinite(a).all() for a in got)
    assert _bits_equal(got, _all_of(r2))


def test_word_axis_on_one_word_is_the_one_word_kernel():
    """train_words with both rows holding the same word and the same draws gives, bit for bit, online_training on that word: the
    word-axis kernel shares the chunk code, the accumulators and the optimizer update with online_train_kernel<256, false>."""
    case = C.CASES["S256_drawn_T136_M33"]
    want = G.run(case, DEV, True, n=2)
    w = G.word_of(case)
    T = case["T"]
    tr = G.trainer_with(G.weights("init", S), S, T, DEV, True)
    y = torch.from_numpy(np.stack([w["y"], w["y"]])).to(DEV)
    tx = torch.from_numpy(np.stack([w["bits"], w["bits"]]).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([G.labels_for(case, w)] * 2)).to(DEV)
    assert tr.words_kernel_route()
    loss = tr._train_words(tx, y, torch.tensor([1, 0], dtype=torch.int32), case["idx"], False, True, labels=lab)
    got = G._state(tr, S, loss)
    assert _bits_equal(_all_of(got), _all_of(want))
