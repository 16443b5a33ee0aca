"""Controlled inputs of the traced-back by-word step (mvn_vnet_byword_step_path_f32 / mvn_va_byword_step_path_f32), from the CPU
oracle alone.  Imported by test_path_step_host.py (which shows that the inputs exercise what they are meant to) and
test_gpu_path_step.py.

  words(T, nsym, R, snr)    R random messages, their RS codewords, and the codewords over codec_cases' static time-decay channel
                            at snr dB: msg = RandomState(5).randint(0, 2, (R, T - 8 nsym)), noise seed = snr.
  costs(kind, y, weights)   the branch costs [R, T, 16] of the ViterbiNet ('vnet': -logits) or Viterbi ('va') detector.
  detect(cost)              (running, path): the reference's running-argmin decisions and the traced-back maximum-likelihood word
                            (oracle.acs_sweep_surv + oracle.traceback).
  expected(kind, ...)       the step on the path: dec and codec_cases.reference_step on it.
  flow_words()              the 12 blocks of the eval_by_word tests: rows of the 8 dB batch chosen so that, with 4 subframes per frame
                            (blocks 0, 4, 8 are pilots), data blocks fail under the path, others under the running argmin only.
"""
import functools

import numpy as np

import codec_cases as C
import oracle

SNRS = (6, 8)
KINDS = ("va", "vnet")
R_HOST, T_HOST, NSYM_HOST = 64, 136, 2  # the reference's word: 120 message bits, RS(17, 15)
FLOW_ROWS = (1, 2, 29, 17, 3, 34, 5, 21, 6, 39, 7, 59)
FLOW_SUBFRAMES = 4


@functools.lru_cache(maxsize=None)
def words(T, nsym, R, snr):
    msg = np.random.RandomState(5).randint(0, 2, (R, T - 8 * nsym)).astype(np.float32)
    cw = oracle.rs_encode_bits(msg, nsym)
    y = C.clean_channel(cw, sigma=10.0 ** (-snr / 20.0), seed=snr)
    return msg, cw, y


def costs(kind, y, weights=None, priors=None):
    if kind == "va":
        return oracle.va_costs(y, C.channel()[1] if priors is None else priors)
    return -oracle.vnet_logits(y, weights)  # vnet_detector.py:57


def detect(cost):
    running, fm, surv = oracle.acs_sweep_surv(cost)
    return running, oracle.traceback(surv, fm)[0]


def expected(kind, y, msg, nsym, weights=None, priors=None):
    """dict(dec, msg, nerr, enc, label_word, labels, status) of the path step, and the running-argmin decisions under 'running'."""
    running, path = detect(costs(kind, y, weights, priors))
    return dict(C.reference_step(path, msg, nsym, False), dec=path, running=running)


def flow_words():
    """(msg [12, 120], y [12, 136]) of the flow tests."""
    msg, _, y = words(T_HOST, NSYM_HOST, R_HOST, 8)
    sel = list(FLOW_ROWS)
    return msg[sel], y[sel]
