"""Words, weights, expected values and a launcher for the by-word block step at 4, 8, 32, 64 and 128 states
(mvn_vnet_byword_step_states_f32, csrc/byword_step_states.inc).  Imported by test_states_step_host.py (CPU) and
test_gpu_states_step.py; everything but launch() runs without a GPU.

  word_set(golden, S)
      S = 8, 32, 64, 128: the 50 received words, messages and starting weights w0 of the reference's own by-word runs, goldens G16
      (L3_selfsup, L5_selfsup) and G17 (L6_selfsup, L7_selfsup): nsym = 2, T = 136.
      S = 4: G3's S4_trained_exact weights (the reference's trainer at memory 2, 10 dB) and 64 coded words over the memory-2 time-decay
      channel, 32 at each of S4_SNRS_DB.  isi_awgn() is mvn.transmit's arithmetic in NumPy float64 (the CPU tests have no device to
      call it on; test_gpu_states_step.py checks that mvn.transmit returns the same words).
  expected_step(dec, msg, nsym, pilot, S)
      codec_cases.reference_step (the C oracle's codec) with the labels taken at the trellis memory log2 S.
  outcomes(golden, S)
      How the oracle's detection and codec end on the word set: clean / corrected / failed words.
  small_case(golden, S, T, nsym, weights)
      Six random coded words of T symbols over the memory-log2(S) time-decay channel at 9 dB with random or the word set's weights.
"""
import ctypes
import functools

import numpy as np

import codec_cases as C
import oracle

STATES = (4, 8, 32, 64, 128)
T_WORD, NSYM_WORD = 136, 2
FLOW = {8: ("g16_by_word_other_state_counts", "L3_selfsup"), 32: ("g16_by_word_other_state_counts", "L5_selfsup"),
        64: ("g17_by_word_64_128_states", "L6_selfsup"), 128: ("g17_by_word_64_128_states", "L7_selfsup")}
# chosen on the oracle alone: outcomes(golden, 4) = 20 clean, 27 corrected, 17 failed words, above the floors the other sets keep
S4_SNRS_DB = (8.5, 9.5)
S4_WORDS = 64
GAMMA = 0.2
ENTRY = "mvn_vnet_byword_step_states_f32"


def memory(S):
    return int(np.log2(S))


def isi_awgn(words, L, snr_db, seed, gamma=GAMMA):
    """y[t] = sum_i h[L-1-i] (1 - 2 c[t+i]) + sigma w[t], h = exp(-gamma arange(L)), c zero-padded by L, sigma = 10^(-snr/20), w
    standard normal from `seed`: float64 in isi_awgn_kernel's order of operations, stored as float32.  Returns (y, w)."""
    c = np.asarray(words, np.float64)
    B, T = c.shape
    h = np.exp(-gamma * np.arange(L))
    s = np.concatenate([1.0 - 2.0 * c, np.ones((B, L))], axis=1)
    y = np.zeros((B, T))
    for i in range(L):
        y += h[L - 1 - i] * s[:, i:i + T]
    w = np.random.RandomState(seed).standard_normal((B, T))
    sigma = (10 ** (snr_db / 10)) ** (-0.5)
    return (y + sigma * w).astype(np.float32), w


@functools.lru_cache(maxsize=None)
def _s4_words():
    oracle.build()
    rng = np.random.RandomState(404)
    msg = rng.randint(0, 2, (S4_WORDS, T_WORD - 8 * NSYM_WORD)).astype(np.float32)
    cw = oracle.rs_encode_bits(msg, NSYM_WORD)
    half = S4_WORDS // 2
    parts = [isi_awgn(cw[i * half:(i + 1) * half], 2, snr, 4040 + i) for i, snr in enumerate(S4_SNRS_DB)]
    return msg, cw, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


_SETS = {}


def word_set(golden, S):
    """dict: rx [R, 136] fp32, msg [R, 120] fp32, cw [R, 136] the codewords sent, w: the six weight arrays, nsym, S."""
    if S not in _SETS:
        oracle.build()
        if S == 4:
            g3 = golden("g3_vnet")
            msg, cw, rx, _ = _s4_words()
            w = [np.ascontiguousarray(g3[f"S4_trained_exact_w{i}"], dtype=np.float32) for i in range(6)]
        else:
            name, tag = FLOW[S]
            g = golden(name)
            msg = np.ascontiguousarray(g[f"{tag}_tx"], dtype=np.float32)
            rx = np.ascontiguousarray(g[f"{tag}_rx"], dtype=np.float32)
            cw = oracle.rs_encode_bits(msg, NSYM_WORD)
            w = [np.ascontiguousarray(g[f"{tag}_w0_{i}"], dtype=np.float32) for i in range(6)]
        assert rx.shape[1] == T_WORD and msg.shape[1] == T_WORD - 8 * NSYM_WORD and w[4].shape == (S, 50)
        _SETS[S] = dict(rx=rx, msg=msg, cw=cw, w=w, nsym=NSYM_WORD, S=S)
    return _SETS[S]


def expected_step(dec, msg, nsym, pilot, S):
    """One block step for every row from the oracle alone: codec_cases.reference_step, the labels at memory log2 S."""
    ref = C.reference_step(dec, msg, nsym, pilot)
    lw = ref["label_word"]
    ref["labels"] = oracle.calculate_states(memory(S), lw).reshape(lw.shape).astype(np.int32)
    return ref


_DETECTED = {}


def detected(golden, S):
    """The oracle's detection of the word set with its weights, and the oracle's step on it (computed once)."""
    if S not in _DETECTED:
        ws = word_set(golden, S)
        dec = oracle.vnet_decode(ws["rx"], ws["w"])
        _DETECTED[S] = (dec, expected_step(dec, ws["msg"], ws["nsym"], False, S))
    return _DETECTED[S]


def outcomes(golden, S):
    """(clean, corrected, failed): words detected without a byte error, words whose detected bytes differ from the codeword's and
    still decode to the message, words with nerr > 0."""
    ws = word_set(golden, S)
    dec, ref = detected(golden, S)
    nbytes = (C.pack(dec) != C.pack(ws["cw"])).sum(axis=1)
    return int(np.sum(nbytes == 0)), int(np.sum((nbytes > 0) & (ref["nerr"] == 0))), int(np.sum(ref["nerr"] > 0))


def random_weights(S, seed):
    """nn.Linear's default initialisation, U(-1/sqrt(fan_in), 1/sqrt(fan_in)), for the six arrays."""
    rng = np.random.RandomState(seed)
    out = []
    for fan_out, fan_in in ((100, 1), (50, 100), (S, 50)):
        b = 1.0 / np.sqrt(fan_in)
        out.append(rng.uniform(-b, b, (fan_out, fan_in)).astype(np.float32))
        out.append(rng.uniform(-b, b, (fan_out,)).astype(np.float32))
    return out


def small_case(golden, S, T, nsym, weights, R=6):
    """dict like word_set's: R random coded words of T symbols at 9 dB; weights 'random' or 'trained' (the word set's)."""
    oracle.build()
    seed = 1000 * S + 10 * T + nsym
    rng = np.random.RandomState(seed)
    msg = rng.randint(0, 2, (R, T - 8 * nsym)).astype(np.float32)
    cw = oracle.rs_encode_bits(msg, nsym)
    rx, _ = isi_awgn(cw, memory(S), 9.0, seed + 1)
    w = random_weights(S, seed + 2) if weights == "random" else word_set(golden, S)["w"]
    return dict(rx=rx, msg=msg, cw=cw, w=w, nsym=nsym, S=S)


def launch(dev, S, rx, tx, nsym, w, pilot=False, want=None, ld=None, w_stride=None, entry=ENTRY):
    """One launch of the states step through the raw ctypes symbol (step_call.step's conventions: outputs pre-filled with SENTINEL
    and returned with their padding, NaN in rx's padding, 7 in tx's; w: six device tensors or pointers)."""
    import torch

    import meta_viterbinet_amd as mvn
    from step_call import OUTPUTS, INT, SENTINEL, padded

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
    front = (*[a if isinstance(a, ctypes.c_void_p) else mvn._lib.ptr(a) for a in w],
             None if w_stride is None else (ctypes.c_int64 * 6)(*w_stride))
    rc = getattr(mvn._lib.load(), entry)(mvn._lib.ptr(rx_d), lds["rx"], mvn._lib.ptr(tx_d), lds["tx"], *front, p("dec"), lds["dec"],
                                         p("msg"), lds["msg"], p("enc"), lds["enc"], p("lw"), lds["lw"], p("labels"), lds["labels"],
                                         p("nerr"), R, T, nsym, 1 if pilot else 0, S, mvn._lib.current_stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {name: t.cpu().numpy() for name, t in out.items()}, row
