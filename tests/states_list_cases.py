"""CPU referee of the by-word LIST step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_list_f32,
csrc/byword_list_states.inc): list_cases.py's definition with 16 replaced by S, NumPy over the C oracle.  Imported by
test_states_list_host.py (CPU) and test_gpu_states_list.py; everything but launch() runs without a GPU.

  soft(cost)                 alpha [R, T + 1, S], beta [R, T + 1, S], delta [R, T] of the branch costs [R, T, S], every operation an
                             np.float32 one: alpha_{t+1}[s] = min over p in {2s % S, (2s + 1) % S} of alpha_t[p] + cost[t][p],
                             beta_t[p] = cost[t][p] + min(beta_{t+1}[p >> 1], beta_{t+1}[(p >> 1) | S / 2]),
                             delta_t = min_{s odd}(alpha_t + beta_t) - min_{s even}(alpha_t + beta_t).
  delta_by_halves(a, b)      the same delta from the alpha HALF-image and gamma_t[h] = min(beta_t[h], beta_t[h + S / 2]): what the
                             kernel computes (asserted equal to soft's on the word sets, on the CPU).
  metrics(cost, words)       M [R, C] = sum_t cost[r, t, state_t(words[r, c])] in ascending t, states at memory log2 S.
  expected(case, m)          the whole step on a case of states_path_cases.word_set / states_step_cases.small_case: dec (the oracle's
                             traced-back path), delta, order, candidates (list_cases.erasure_fill), metrics, choice and the oracle's
                             codec on the chosen codeword, label word = dec where the chosen message has bit errors, labels at memory
                             log2 S.
  expected_set(golden, S, m) expected() of the word set, computed once.
"""
import itertools

import numpy as np

import list_cases as LC
import oracle
import states_path_cases as PC
import states_step_cases as SC

f32 = np.float32
ENTRY = "mvn_vnet_byword_step_states_list_f32"
PATH_ENTRY = PC.ENTRY
RUNNING_ENTRY = SC.ENTRY
OUTPUTS = ("dec", "delta", "choice", "msg", "nerr", "enc", "lw", "labels")


def soft(cost):
    cost = np.ascontiguousarray(cost, dtype=f32)
    R, T, S = cost.shape
    s = np.arange(S)
    p0, p1 = (2 * s) % S, (2 * s + 1) % S
    n0, n1 = s >> 1, (s >> 1) | (S // 2)
    alpha = np.zeros((R, T + 1, S), f32)
    for t in range(T):
        a = alpha[:, t] + cost[:, t]
        assert a.dtype == f32
        alpha[:, t + 1] = np.minimum(a[:, p0], a[:, p1])
    beta = np.zeros((R, T + 1, S), f32)
    for t in range(T - 1, -1, -1):
        beta[:, t] = cost[:, t] + np.minimum(beta[:, t + 1][:, n0], beta[:, t + 1][:, n1])
    ab = alpha[:, :T] + beta[:, :T]
    delta = ab[:, :, 1::2].min(axis=2) - ab[:, :, 0::2].min(axis=2)
    assert ab.dtype == f32 and delta.dtype == f32
    return alpha, beta, delta


def delta_by_halves(alpha, beta):
    """delta [R, T] from alpha[..., :S / 2] and gamma = min(beta[..., :S / 2], beta[..., S / 2:]), fp32."""
    T, H = alpha.shape[1] - 1, alpha.shape[2] // 2
    ab = alpha[:, :T, :H] + np.minimum(beta[:, :T, :H], beta[:, :T, H:])
    assert ab.dtype == f32
    return ab[:, :, 1::2].min(axis=2) - ab[:, :, 0::2].min(axis=2)


def metrics(cost, words):
    R, Cn, T = words.shape
    L = SC.memory(cost.shape[2])
    st = oracle.calculate_states(L, words.reshape(R * Cn, T).astype(f32)).reshape(R, Cn, T).astype(np.int64)
    M = np.zeros((R, Cn), f32)
    rr = np.arange(R)[:, None]
    for t in range(T):
        M = M + cost[rr, t, st[:, :, t]]
    assert M.dtype == f32
    return M


def expected(case, m, w=None):
    """case: a dict of word_set / small_case; w: other weights than the case's (a list of six arrays, or one such list per word)."""
    rx, msg, nsym, S = case["rx"], case["msg"], case["nsym"], case["S"]
    w = case["w"] if w is None else w
    if isinstance(w[0], (list, tuple)):  # a weight set per word
        cost = np.concatenate([-oracle.vnet_logits(rx[r:r + 1], w[r]) for r in range(rx.shape[0])])
        dec = np.concatenate([PC.path(rx[r:r + 1], w[r]) for r in range(rx.shape[0])])
    else:
        cost = -oracle.vnet_logits(rx, w)
        dec = PC.path(rx, w)
    cost = np.ascontiguousarray(cost, dtype=f32)
    R, T, _ = cost.shape
    n = T // 8
    alpha, beta, delta = soft(cost)
    rho = np.abs(delta).reshape(R, n, 8).min(axis=2)
    order = np.argsort(rho, axis=1, kind="stable")  # (rho, j) ascending
    hard = oracle.rs_encode_bits(oracle.rs_decode_bits(np.ascontiguousarray(dec, dtype=f32), nsym), nsym)
    subsets = list(itertools.combinations(range(m), nsym))
    cands = np.zeros((R, 1 + len(subsets), T), f32)
    cands[:, 0] = hard
    for r in range(R):
        for c, sub in enumerate(subsets):
            cands[r, 1 + c] = LC.erasure_fill(dec[r], order[r, list(sub)], nsym)
    M = metrics(cost, cands)
    choice = np.argmin(M, axis=1).astype(np.int32)  # the first minimum
    chosen = cands[np.arange(R), choice]
    step = SC.expected_step(chosen, msg, nsym, False, S)
    assert np.array_equal(step["enc"], chosen)  # a codeword decodes to itself
    lw = np.where((step["nerr"] > 0)[:, None], dec, step["enc"]).astype(f32)
    labels = oracle.calculate_states(SC.memory(S), lw).reshape(lw.shape).astype(np.int32)
    path_step = SC.expected_step(dec, msg, nsym, False, S)
    return dict(dec=dec, alpha=alpha, beta=beta, delta=delta, order=order, candidates=cands, metrics=M, choice=choice, msg=step["msg"],
                nerr=step["nerr"], enc=step["enc"], lw=lw, labels=labels, path_nerr=path_step["nerr"])


_EXPECTED = {}


def expected_set(golden, S, m=4):
    if (S, m) not in _EXPECTED:
        _EXPECTED[S, m] = expected(PC.word_set(golden, S), m)
    return _EXPECTED[S, m]


def launch(dev, S, rx, tx, nsym, m, w, pilot=False, want=None, ld=None, w_stride=None, entry=ENTRY):
    """One launch of the list states step through the raw ctypes symbol, states_step_cases.launch's conventions (outputs pre-filled with
    their sentinels and returned with their padding, NaN in rx's padding, 7 in tx's); tx None on a data step: no transmitted word."""
    import ctypes

    import torch

    import meta_viterbinet_amd as mvn
    from step_call import INT, SENTINEL, padded

    R = tx.shape[0] if rx is None else rx.shape[0]
    T = tx.shape[1] + 8 * nsym if rx is None else rx.shape[1]
    K = T - 8 * nsym
    row = {"rx": T, "tx": K, "dec": T, "msg": K, "enc": T, "lw": T, "labels": T, "delta": T}
    lds = dict(row, **(ld or {}))
    rx_d = None if rx is None else padded(rx, lds["rx"], np.nan, dev)
    tx_d = None if tx is None else padded(tx, lds["tx"], 7.0, dev)
    want = OUTPUTS if want is None else tuple(want)
    out = {}
    for name in want:
        shape = (R,) if name in ("nerr", "choice") else (R, lds[name])
        out[name] = torch.full(shape, SENTINEL[name], dtype=torch.int32 if name in INT else torch.float32, device=dev)
    p = lambda name: mvn._lib.ptr(out.get(name))  # noqa: E731
    front = (*[a if isinstance(a, ctypes.c_void_p) else mvn._lib.ptr(a) for a in w],
             None if w_stride is None else (ctypes.c_int64 * 6)(*w_stride))
    rc = getattr(mvn._lib.load(), entry)(mvn._lib.ptr(rx_d), lds["rx"], mvn._lib.ptr(tx_d), lds["tx"], *front, p("dec"), lds["dec"],
                                         p("msg"), lds["msg"], p("enc"), lds["enc"], p("lw"), lds["lw"], p("labels"), lds["labels"],
                                         p("nerr"), R, T, nsym, 1 if pilot else 0, S, m, p("delta"), lds["delta"], p("choice"),
                                         mvn._lib.current_stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {name: t.cpu().numpy() for name, t in out.items()}, row
