"""Shared by tests/test_gpu_vnet_grad_256.py and tests/test_vnet_grad_256_host.py (no tests of its own): tests/vnet_grad_cases.py's
online table once more at 256 states, for online_train_kernel<256, false> and online_train_words_states256_kernel, whose W3
gradient lives in MFMA accumulators across a pass instead of in the LDS gradient vector (csrc/online_train.inc, grad_chunk).

Same shapes, draws, referee, bound and margin as at every other state count -- the cases are built by vnet_grad_cases._online and
read through its checks.  One thing that module does for its own table only is done here: the word of a second-iteration case must
also clear the ReLU margin at the weights after step 1, and vnet_grad_cases.word_of looks for such cases in its own ONLINE table.
words() draws the words of this table the way word_of does (the same generator and seed per (S, T), _draw_word, _clean) with the
second-iteration cases of THIS table as the ones whose stepped weights count, and places them in vnet_grad_cases._WORDS, where
word_of, run and reference_of find them.  Every test module calls words() before it touches a case."""
import numpy as np
import torch

import vnet_grad_cases as G

S = 256


def _table():
    out = []
    for T in G.WHOLE_T:
        out.append(G._online(f"whole_T{T}", S, T, second=T in (33, 136)))
    for M in G.MINIBATCH_M:
        second = M in (32, 33)
        out.append(G._online(f"drawn_T136_M{M}", S, 136, G.draw(136, M, 1 + second, 2000 * S + M), second=second))
    out.append(G._online("dup_T136", S, 136, G.DUPLICATES))
    out.append(G._online("perm_T64_M64", S, 64, np.random.RandomState(64 + S).permutation(64).reshape(1, 64)))
    out.append(G._online("same_label_T33", S, 33, labels="same"))
    return out


CASES = {c["name"]: c for c in _table()}
NAMES = list(CASES)
SECOND_NAMES = [n for n in NAMES if CASES[n]["second"]]


def words():
    """Places this table's words in vnet_grad_cases._WORDS (once per process)."""
    for T in sorted({c["T"] for c in CASES.values()}):
        key = (S, T, "init")
        if key in G._WORDS:
            continue
        rng = np.random.RandomState(100000 + 1000 * G.memory_length(S) + T)
        sigma = G.SIGMA["init"]
        bits, y = G._draw_word(rng, S, T, sigma)
        ws = G.weights("init", S)
        every = np.ones(T, bool)

        def stepped(c):
            def cond(y_):
                lab = G.labels_for(c, dict(states=G.states_of(bits, S)))
                g, _ = G.torch_gradient(ws, y_, lab, None if c["idx"] is None else c["idx"][0], torch.float64)
                return [(G.adam_step1(ws, g), every, 2 * G.RELU_MARGIN)]
            return cond

        users = [c for c in CASES.values() if c["T"] == T and c["second"]]
        y = G._clean(rng, y, bits, sigma, [(ws, every, G.KEEP_CLEAR)], [stepped(c) for c in users], f"word {key}")
        G._WORDS[key] = dict(bits=bits, y=y, states=G.states_of(bits, S))


def samples_of(case):
    return case["T"] if case["idx"] is None else case["idx"].shape[1]
