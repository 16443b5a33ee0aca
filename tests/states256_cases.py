"""Words, weights, priors, expected values and a launcher for the by-word block steps at 256 states (mvn_vnet_byword_step_256_f32,
_256_path_f32, mvn_va_byword_step_256_f32, _256_path_f32; csrc/byword_step_256.inc).  Imported by test_states256_host.py (CPU) and
test_gpu_states256_step.py; everything but launch() runs without a GPU.

Expected values come from the C oracle only:
  ViterbiNet running   oracle.vnet_decode
  ViterbiNet path      oracle.vnet_logits -> oracle.acs_sweep_surv(-logits) -> oracle.traceback
  classical            va_states_cases.expected (oracle.va_costs / va_decode / acs_sweep_surv / traceback)
  codec                states_step_cases.expected_step(..., S=256): the oracle's codec, the labels at memory 8

  vnet_word_set(golden)  82 words of 136 symbols, RS(17, 15): the 50 received words, messages and starting weights of golden G23 (the
                         reference's own by-word run at memory 8) and 32 more, random messages (RandomState(2560)) sent with
                         states_step_cases.isi_awgn over the memory-8 time-decay channel at 14 dB (noise seed 25614), G23's weights
  va_word_set()          va_states_cases.word_set(256): 48 words, 24 at 6 dB and 24 at 8 dB
  vnet_small_case / va_small_case   a few random coded words of T symbols
"""
import ctypes

import numpy as np

import codec_cases as C
import oracle
import states_step_cases as SC
import va_states_cases as VC

f32 = np.float32
S = 256
MEMORY = 8
T_WORD, NSYM_WORD = SC.T_WORD, SC.NSYM_WORD
GOLDEN, TAG = "g23_by_word_256_states", "L8_selfsup"
EXTRA_WORDS, EXTRA_SNR_DB = 32, 14.0
ENTRY = {("vnet", "running"): "mvn_vnet_byword_step_256_f32", ("vnet", "path"): "mvn_vnet_byword_step_256_path_f32",
         ("va", "running"): "mvn_va_byword_step_256_f32", ("va", "path"): "mvn_va_byword_step_256_path_f32"}
KINDS, DECISIONS = ("vnet", "va"), ("running", "path")
OUTPUTS = ("dec", "msg", "enc", "lw", "labels", "nerr")

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def vnet_word_set(golden):
    """dict: rx [82, 136] fp32, msg [82, 120], cw [82, 136], w: G23's six starting weight arrays, nsym, S."""
    def make():
        oracle.build()
        g = golden(GOLDEN)
        w = [np.ascontiguousarray(g[f"{TAG}_w0_{i}"], dtype=f32) for i in range(6)]
        msg = np.ascontiguousarray(g[f"{TAG}_tx"], dtype=f32)
        rx = np.ascontiguousarray(g[f"{TAG}_rx"], dtype=f32)
        more = np.random.RandomState(2560).randint(0, 2, (EXTRA_WORDS, T_WORD - 8 * NSYM_WORD)).astype(f32)
        more_rx = SC.isi_awgn(oracle.rs_encode_bits(more, NSYM_WORD), MEMORY, EXTRA_SNR_DB, 25614)[0]
        msg, rx = np.concatenate([msg, more]), np.concatenate([rx, more_rx])
        assert rx.shape == (82, T_WORD) and msg.shape == (82, T_WORD - 8 * NSYM_WORD) and w[4].shape == (S, 50)
        return dict(rx=rx, msg=msg, cw=oracle.rs_encode_bits(msg, NSYM_WORD), w=w, nsym=NSYM_WORD, S=S)
    return _once("vnet_set", make)


def va_word_set():
    return VC.word_set(S)


def vnet_path(rx, w):
    logits = oracle.vnet_logits(np.ascontiguousarray(rx, dtype=f32), w)
    _, fm, surv = oracle.acs_sweep_surv(np.ascontiguousarray(-logits, dtype=f32))
    return oracle.traceback(surv, fm)[0]


def vnet_detect(rx, w, decision):
    return oracle.vnet_decode(rx, w) if decision == "running" else vnet_path(rx, w)


def expected(kind, case, decision):
    """dict: dec, msg, nerr, enc, lw, labels of the step on a case (vnet: rx, msg, w, nsym; va: rx, msg, pri, nsym, S)."""
    if kind == "va":
        return VC.expected(case, decision)
    dec = vnet_detect(case["rx"], case["w"], decision)
    ref = SC.expected_step(dec, case["msg"], case["nsym"], False, S)
    return dict(dec=dec, msg=ref["msg"], nerr=ref["nerr"], enc=ref["enc"], lw=ref["label_word"], labels=ref["labels"])


def expected_set(golden, kind, decision):
    return _once(("exp", kind, decision),
                 lambda: expected(kind, vnet_word_set(golden) if kind == "vnet" else va_word_set(), decision))


def expected_pilot(tx, nsym):
    return VC.expected_pilot(tx, nsym, S)


def outcomes(golden, kind, decision):
    """(clean, corrected, failed) words: detected without a byte error; detected bytes differ from the codeword's and still decode to
    the message; nerr > 0."""
    ws = vnet_word_set(golden) if kind == "vnet" else va_word_set()
    exp = expected_set(golden, kind, decision)
    nbytes = (C.pack(exp["dec"]) != C.pack(ws["cw"])).sum(axis=1)
    return int(np.sum(nbytes == 0)), int(np.sum((nbytes > 0) & (exp["nerr"] == 0))), int(np.sum(exp["nerr"] > 0))


def vnet_small_case(golden, T, nsym, weights, R=3):
    """R random coded words of T symbols at 9 dB over the memory-8 channel; weights 'random' (nn.Linear's initialisation) or
    'trained' (G23's)."""
    oracle.build()
    seed = 1000 * S + 10 * T + nsym
    msg = np.random.RandomState(seed).randint(0, 2, (R, T - 8 * nsym)).astype(f32)
    cw = oracle.rs_encode_bits(msg, nsym)
    rx, _ = SC.isi_awgn(cw, MEMORY, 9.0, seed + 1)
    w = SC.random_weights(S, seed + 2) if weights == "random" else vnet_word_set(golden)["w"]
    return dict(rx=rx, msg=msg, cw=cw, w=w, nsym=nsym, S=S)


def va_small_case(T, nsym, R=3, gammas=(VC.GAMMA,)):
    return VC.small_case(S, T, nsym, R=R, gammas=gammas)


def launch(dev, kind, decision, rx, tx, nsym, front, pilot=False, want=None, ld=None, w_stride=None, n_states=S):
    """One launch of mvn_{kind}_byword_step_256[_path]_f32 through the raw ctypes symbol, step_call.step's conventions: the outputs
    pre-filled with SENTINEL and returned with their padding, NaN in rx's padding, 7 in tx's.  rx: a host array or None (NULL: R and T
    from tx).  front: vnet -- six device tensors or pointers (w_stride: six strides or None); va -- a host array [Bp, 256] or None
    (NULL, Bp = 1).  Returns (outputs, row lengths)."""
    import torch

    import meta_viterbinet_amd as mvn
    from step_call import INT, SENTINEL, padded

    R = tx.shape[0] if rx is None else rx.shape[0]
    T = tx.shape[1] + 8 * nsym if rx is None else rx.shape[1]
    K = T - 8 * nsym
    row = {"rx": T, "tx": K, "dec": T, "msg": K, "enc": T, "lw": T, "labels": T}
    lds = dict(row, **(ld or {}))
    rx_d = None if rx is None else padded(rx, lds["rx"], np.nan, dev)
    tx_d = padded(tx, lds["tx"], 7.0, dev)
    want = OUTPUTS if want is None else tuple(want)
    out = {}
    for name in want:
        shape = (R,) if name == "nerr" else (R, lds[name])
        out[name] = torch.full(shape, SENTINEL[name], dtype=torch.int32 if name in INT else torch.float32, device=dev)
    p = lambda name: mvn._lib.ptr(out.get(name))  # noqa: E731
    if kind == "va":
        pri_d = None if front is None else torch.as_tensor(np.ascontiguousarray(front, dtype=f32)).to(dev)
        head = (mvn._lib.ptr(pri_d), 1 if front is None else front.shape[0])
    else:
        head = (*[a if isinstance(a, ctypes.c_void_p) else mvn._lib.ptr(a) for a in front],
                None if w_stride is None else (ctypes.c_int64 * 6)(*w_stride))
    rc = getattr(mvn._lib.load(), ENTRY[kind, decision])(
        mvn._lib.ptr(rx_d), lds["rx"], mvn._lib.ptr(tx_d), lds["tx"], *head, p("dec"), lds["dec"], p("msg"), lds["msg"], p("enc"),
        lds["enc"], p("lw"), lds["lw"], p("labels"), lds["labels"], p("nerr"), R, T, nsym, 1 if pilot else 0, n_states,
        mvn._lib.current_stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {name: t.cpu().numpy() for name, t in out.items()}, row
