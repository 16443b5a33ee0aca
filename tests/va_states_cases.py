"""Words, state priors, expected values and a launcher for the classical Viterbi detector's by-word block steps at 4, 8, 32, 64 and
128 states (mvn_va_byword_step_states_f32, _path_f32, _list_f32; csrc/byword_step_states_va.inc).  Imported by
test_va_states_host.py (CPU) and test_gpu_va_states_step.py; everything but launch() runs without a GPU.

Expected values come from the C oracle and the existing referees only:
  cost      oracle.va_costs(rx, priors)                                  (va_detector.py:64-68)
  running   oracle.va_decode: acs_sweep's running-argmin decisions
  path      oracle.acs_sweep_surv(cost) -> oracle.traceback(surv, final)
  codec     states_step_cases.expected_step (the oracle's codec, labels at memory log2 S)
  list      states_list_cases.soft / delta_by_halves / metrics and list_cases.erasure_fill on that cost, in the order
            states_list_cases.expected uses

  priors(S, gamma)       compute_state_priors' arithmetic on h = exp(-gamma arange(log2 S)): [1, S] fp32
  word_set(S)            48 random 120-bit messages (RandomState(100 + S)), RS(17, 15)-encoded (T = 136, nsym = 2), sent with
                         states_step_cases.isi_awgn over the memory-log2(S) time-decay channel: 24 words at 6.0 dB (noise seed
                         500 + S) and 24 at 8.0 dB (noise seed 501 + S).  At 8 / 10 dB the path never fails at 4 and 8 states.
  expected(case, decision, m)
                         the whole step on a case (a dict with rx, msg, pri, nsym, S)
  expected_set(S, decision)   expected() of the word set, computed once
  outcomes(S, decision)  (clean, corrected, failed) words as states_step_cases.outcomes counts them
  small_case(S, T, nsym, R, gammas)   R random coded words of T symbols at 7 dB, word r on the channel of gammas[r % len(gammas)]
"""
import itertools

import numpy as np

import codec_cases as C
import list_cases as LC
import oracle
import states_list_cases as LSC
import states_step_cases as SC

f32 = np.float32
STATES = SC.STATES
T_WORD, NSYM_WORD = SC.T_WORD, SC.NSYM_WORD
WORDS, SNRS_DB = 48, (6.0, 8.0)
GAMMA = SC.GAMMA
LIST_BYTES = 4
ENTRY = {"running": "mvn_va_byword_step_states_f32", "path": "mvn_va_byword_step_states_path_f32",
         "list": "mvn_va_byword_step_states_list_f32"}
OUTPUTS = ("dec", "msg", "enc", "lw", "labels", "nerr")
LIST_OUTPUTS = OUTPUTS + ("delta", "choice")


def priors(S, gamma=GAMMA, h=None):
    """[1, S] fp32: VADetector.compute_state_priors (va_detector.py:42-50) of the time-decay channel h = exp(-gamma arange(L)), or of
    the L taps given."""
    L = SC.memory(S)
    h = (np.exp(-gamma * np.arange(L)) if h is None else np.asarray(h, np.float64)).reshape(1, L)
    binary = np.unpackbits(np.arange(S).astype(np.uint8).reshape(-1, 1), axis=1).astype(int)
    symbols = 1 - 2 * binary[:, -L:]
    return np.ascontiguousarray(np.dot(symbols, h.T).T, dtype=f32)


_SETS = {}


def word_set(S):
    """dict: rx [48, 136] fp32, msg [48, 120], cw [48, 136], pri [1, S], nsym, S."""
    if S not in _SETS:
        oracle.build()
        msg = np.random.RandomState(100 + S).randint(0, 2, (WORDS, T_WORD - 8 * NSYM_WORD)).astype(f32)
        cw = oracle.rs_encode_bits(msg, NSYM_WORD)
        half = WORDS // 2
        rx = np.concatenate([SC.isi_awgn(cw[i * half:(i + 1) * half], SC.memory(S), snr, 500 + S + i)[0] for i, snr in enumerate(SNRS_DB)])
        _SETS[S] = dict(rx=rx, msg=msg, cw=cw, pri=priors(S), nsym=NSYM_WORD, S=S)
    return _SETS[S]


def costs(case):
    return np.ascontiguousarray(oracle.va_costs(case["rx"], case["pri"]), dtype=f32)


def running(case):
    return oracle.va_decode(case["rx"], case["pri"], want_final=False)


def path(case):
    _, fm, surv = oracle.acs_sweep_surv(costs(case))
    return oracle.traceback(surv, fm)[0]


def expected(case, decision, m=LIST_BYTES):
    """dict: dec, msg, nerr, enc, lw, labels of the step; 'list' adds delta, choice, alpha, beta, candidates, metrics and path_nerr
    (the path step's error counts).  A pilot: expected_pilot()."""
    msg, nsym, S = case["msg"], case["nsym"], case["S"]
    if decision in ("running", "path"):
        dec = running(case) if decision == "running" else path(case)
        ref = SC.expected_step(dec, msg, nsym, False, S)
        return dict(dec=dec, msg=ref["msg"], nerr=ref["nerr"], enc=ref["enc"], lw=ref["label_word"], labels=ref["labels"])
    cost = costs(case)
    dec = path(case)
    R, T, _ = cost.shape
    n = T // 8
    alpha, beta, delta = LSC.soft(cost)
    rho = np.abs(delta).reshape(R, n, 8).min(axis=2)
    order = np.argsort(rho, axis=1, kind="stable")  # (rho, j) ascending
    hard = oracle.rs_encode_bits(oracle.rs_decode_bits(np.ascontiguousarray(dec, dtype=f32), nsym), nsym)
    subsets = list(itertools.combinations(range(m), nsym))
    cands = np.zeros((R, 1 + len(subsets), T), f32)
    cands[:, 0] = hard
    for r in range(R):
        for c, sub in enumerate(subsets):
            cands[r, 1 + c] = LC.erasure_fill(dec[r], order[r, list(sub)], nsym)
    M = LSC.metrics(cost, cands)
    choice = np.argmin(M, axis=1).astype(np.int32)  # the first minimum
    chosen = cands[np.arange(R), choice]
    step = SC.expected_step(chosen, msg, nsym, False, S)
    assert np.array_equal(step["enc"], chosen)  # a codeword decodes to itself
    lw = np.where((step["nerr"] > 0)[:, None], dec, step["enc"]).astype(f32)
    labels = oracle.calculate_states(SC.memory(S), lw).reshape(lw.shape).astype(np.int32)
    path_step = SC.expected_step(dec, msg, nsym, False, S)
    return dict(dec=dec, alpha=alpha, beta=beta, delta=delta, order=order, candidates=cands, metrics=M, choice=choice, msg=step["msg"],
                nerr=step["nerr"], enc=step["enc"], lw=lw, labels=labels, path_nerr=path_step["nerr"])


def expected_pilot(tx, nsym, S):
    ref = SC.expected_step(None, tx, nsym, True, S)
    return dict(dec=None, msg=None, nerr=ref["nerr"], enc=ref["enc"], lw=ref["label_word"], labels=ref["labels"])


_EXPECTED = {}


def expected_set(S, decision):
    if (S, decision) not in _EXPECTED:
        _EXPECTED[S, decision] = expected(word_set(S), decision)
    return _EXPECTED[S, decision]


def outcomes(S, decision):
    """(clean, corrected, failed): words detected without a byte error, words whose detected bytes differ from the codeword's and
    still decode to the message, words with nerr > 0 -- of the running or the path detection and the hard decoder."""
    ws = word_set(S)
    exp = expected_set(S, decision)
    nbytes = (C.pack(exp["dec"]) != C.pack(ws["cw"])).sum(axis=1)
    return int(np.sum(nbytes == 0)), int(np.sum((nbytes > 0) & (exp["nerr"] == 0))), int(np.sum(exp["nerr"] > 0))


def small_case(S, T, nsym, R=6, gammas=(GAMMA,), snr_db=7.0):
    """dict like word_set's: R random coded words of T symbols; word r travels the channel of gamma gammas[r % len(gammas)] and
    pri [len(gammas), S] holds that channel's priors in row r % len(gammas)."""
    oracle.build()
    seed = 2000 * S + 10 * T + nsym + 7 * len(gammas)
    msg = np.random.RandomState(seed).randint(0, 2, (R, T - 8 * nsym)).astype(f32)
    cw = oracle.rs_encode_bits(msg, nsym)
    rx = np.concatenate([SC.isi_awgn(cw[r:r + 1], SC.memory(S), snr_db, seed + 1 + r, gamma=gammas[r % len(gammas)])[0] for r in range(R)])
    pri = np.concatenate([priors(S, g) for g in gammas])
    return dict(rx=rx, msg=msg, cw=cw, pri=pri, nsym=nsym, S=S)


def launch(dev, decision, S, rx, tx, nsym, pri, pilot=False, m=LIST_BYTES, want=None, ld=None):
    """One launch of mvn_va_byword_step_states[_path|_list]_f32 through the raw ctypes symbol, step_call.step's conventions: the
    outputs pre-filled with SENTINEL and returned with their padding, NaN in rx's padding, 7 in tx's.  rx / tx: host arrays (None:
    NULL; rx None takes R and T from tx); pri: a host array [Bp, S] or None (NULL, Bp = 1).  Returns (outputs, row lengths)."""
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
    pri_d = None if pri is None else torch.as_tensor(np.ascontiguousarray(pri, dtype=f32)).to(dev)
    has = LIST_OUTPUTS if decision == "list" else OUTPUTS
    want = has if want is None else tuple(n for n in want if n in has)
    out = {}
    for name in want:
        shape = (R,) if name in ("nerr", "choice") else (R, lds[name])
        out[name] = torch.full(shape, SENTINEL[name], dtype=torch.int32 if name in INT else torch.float32, device=dev)
    p = lambda name: mvn._lib.ptr(out.get(name))  # noqa: E731
    tail = (m, p("delta"), lds["delta"], p("choice")) if decision == "list" else ()
    rc = getattr(mvn._lib.load(), ENTRY[decision])(mvn._lib.ptr(rx_d), lds["rx"], mvn._lib.ptr(tx_d), lds["tx"], mvn._lib.ptr(pri_d),
                                                   1 if pri is None else pri.shape[0], p("dec"), lds["dec"], p("msg"), lds["msg"],
                                                   p("enc"), lds["enc"], p("lw"), lds["lw"], p("labels"), lds["labels"], p("nerr"), R, T,
                                                   nsym, 1 if pilot else 0, S, *tail, mvn._lib.current_stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {name: t.cpu().numpy() for name, t in out.items()}, row
