"""Words and expected values for the by-word PATH step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_path_f32,
csrc/byword_step_states.inc), next to states_step_cases.py, whose word sets, small cases and launcher it reuses.  Imported by
test_states_path_host.py (CPU) and test_gpu_states_path.py; nothing here needs a GPU.

  word_set(golden, S)
      S = 8, 32, 64, 128: states_step_cases.word_set, the reference's own 50 words and starting weights.
      S = 4: the running set's messages and weights at lower SNR -- under the path that set leaves no failed word (56 clean, 8 corrected,
      0 failed); this one gives 32 / 20 / 12.
  path(rx, w)
      The traced-back word from the C oracle alone: vnet_logits -> acs_sweep_surv(-logits) -> traceback.
  detected(golden, S)
      (path, running decisions, the oracle's step on the path) of the word set, computed once.
  outcomes(golden, S)
      (clean, corrected, failed) under the path, as states_step_cases.outcomes counts them.
"""
import functools

import numpy as np

import codec_cases as C
import oracle
import states_step_cases as SC

ENTRY = "mvn_vnet_byword_step_states_path_f32"
RUNNING_ENTRY = SC.ENTRY
S4_SNRS_DB = (6.0, 7.0)


@functools.lru_cache(maxsize=None)
def _s4_rx():
    oracle.build()
    msg, cw, _, _ = SC._s4_words()
    half = SC.S4_WORDS // 2
    return msg, cw, np.concatenate([SC.isi_awgn(cw[i * half:(i + 1) * half], 2, snr, 4140 + i)[0] for i, snr in enumerate(S4_SNRS_DB)])


def word_set(golden, S):
    """dict like states_step_cases.word_set's."""
    ws = SC.word_set(golden, S)
    if S != 4:
        return ws
    msg, cw, rx = _s4_rx()
    return dict(ws, rx=rx, msg=msg, cw=cw)


def path(rx, w):
    """bits [B, T]: the oracle's survivors of the oracle's logits, walked back by the oracle."""
    _, fm, surv = oracle.acs_sweep_surv(-oracle.vnet_logits(rx, w))
    return oracle.traceback(surv, fm)[0]


_DETECTED = {}


def detected(golden, S):
    if S not in _DETECTED:
        ws = word_set(golden, S)
        dec = path(ws["rx"], ws["w"])
        _DETECTED[S] = (dec, oracle.vnet_decode(ws["rx"], ws["w"]), SC.expected_step(dec, ws["msg"], ws["nsym"], False, S))
    return _DETECTED[S]


def outcomes(golden, S):
    ws = word_set(golden, S)
    dec, _, ref = detected(golden, S)
    nbytes = (C.pack(dec) != C.pack(ws["cw"])).sum(axis=1)
    return int(np.sum(nbytes == 0)), int(np.sum((nbytes > 0) & (ref["nerr"] == 0))), int(np.sum(ref["nerr"] > 0))
