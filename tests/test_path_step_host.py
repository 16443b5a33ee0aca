"""CPU only: what the traced-back by-word step (mvn_vnet_byword_step_path_f32 / mvn_va_byword_step_path_f32) is tested on, and what of it
can be tested without a device.

  * The controlled inputs of tests/path_cases.py, on the oracle alone: at 6 and 8 dB the path's word differs from the running-argmin
    word in most blocks, leaves fewer failed words, and still leaves some (the 'label word = detected word' branch and decoder
    status 1 are reached).  These are conditions on the inputs, not measurements; tests/test_gpu_path_step.py asserts that the
    GPU's error counts on the same batches equal the oracle's, so the floors carry over.
  * (Argument validation of both entry points: tests/test_step_validation_host.py, the table over all six block steps.)
  * The new kernels in the gfx950 code object: they exist, use no scratch, and the ViterbiNet form (which shares the 16-wave
    workgroup's occupancy step) keeps to 128 VGPRs."""
import re

import numpy as np
import pytest

import exact_nets
import meta_viterbinet_amd as mvn
import path_cases as P
from test_kernel_resources import resources  # noqa: F401  (the fixture that reads the built library's code object)


@pytest.fixture(scope="module")
def batches(oracle, golden):
    import codec_cases as C

    w = C.g7_weights(golden)
    out = {}
    for snr in P.SNRS:
        msg, cw, y = P.words(P.T_HOST, P.NSYM_HOST, P.R_HOST, snr)
        for kind in P.KINDS:
            exp = P.expected(kind, y, msg, P.NSYM_HOST, weights=w)
            run = C.reference_step(exp["running"], msg, P.NSYM_HOST, False)
            out[snr, kind] = dict(exp=exp, run=run, cw=cw)
    return out


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_path_and_running_words_differ_and_the_path_fails_less(batches, snr, kind):
    b = batches[snr, kind]
    differ = int(np.any(b["exp"]["dec"] != b["exp"]["running"], axis=1).sum())
    wrong_run, wrong_path = int((b["run"]["nerr"] > 0).sum()), int((b["exp"]["nerr"] > 0).sum())
    raw_run, raw_path = int((b["exp"]["running"] != b["cw"]).sum()), int((b["exp"]["dec"] != b["cw"]).sum())
    print(f"{snr} dB {kind}: {differ} words differ, raw bit errors {raw_run} / {raw_path}, failed words {wrong_run} / {wrong_path}")
    assert differ >= 40
    assert wrong_run >= 12
    assert 4 <= wrong_path < wrong_run


def test_path_words_reach_decoder_status_1(batches):
    n = sum(int((b["exp"]["status"] == 1).sum()) for b in batches.values())
    assert n >= 3, n


@pytest.mark.parametrize("kind", P.KINDS)
def test_flow_words_fail_differently_under_the_two_rules(oracle, golden, kind):
    """The 12 blocks of the eval_by_word tests (with the weights the runs start from): among the data blocks at least two fail under
    the path, and at least one fails under the running argmin alone."""
    import codec_cases as C

    msg, y = P.flow_words()
    exp = P.expected(kind, y, msg, P.NSYM_HOST, weights=C.g7_weights(golden))
    run = C.reference_step(exp["running"], msg, P.NSYM_HOST, False)
    data = np.arange(len(P.FLOW_ROWS)) % P.FLOW_SUBFRAMES != 0
    assert int((exp["nerr"][data] > 0).sum()) >= 2
    assert int(((run["nerr"] > 0) & (exp["nerr"] == 0))[data].sum()) >= 1


def test_tie_cases_hold_a_tied_final_minimum():
    """(precondition of test_gpu_path_step.py::test_path_step_breaks_ties_like_torch, NumPy only) at least one block ends with its minimal final metric in two states."""
    n = 0
    for fast in (True, False):
        for B, T in [(5, 136), (3, 200), (70, 72)]:
            fm = exact_nets.tie_case(16, fast, False, B, T)["fm"]
            n += int(np.sum((fm == fm.min(axis=1, keepdims=True)).sum(axis=1) > 1))
    assert n >= 1, n


def test_path_step_kernels_resources(resources):  # noqa: F811
    for pattern, budget in ((r"byword_path_step_kernel<(2|8)>", 128), (r"byword_path_step_va_kernel<(2|8)>", None)):
        names = [n for n in resources if re.fullmatch(pattern, n)]
        assert len(names) == 2, f"{pattern}: {names}"
        for n in names:
            print(n, resources[n])
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            if budget is not None:
                assert resources[n]["vgpr"] <= budget, f"{n}: {resources[n]['vgpr']} VGPRs, built for <= {budget}"


def test_decision_keyword_is_validated():
    import torch

    from meta_viterbinet_amd.lstm import LSTMDetector

    det = mvn.VNETDetector(16, {"train": 136, "val": 136})
    tx, rx = torch.zeros(2, 120), torch.zeros(2, 136)
    with pytest.raises(ValueError, match="decision"):
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="traceback")
    with pytest.raises(ValueError, match="path"):
        mvn.eval_by_word(LSTMDetector(), tx, rx, 8.0, 0.2, 2, 4, decision="path")
    with pytest.raises(ValueError, match="decision"):
        mvn.eval_counters(det, tx, rx, 8.0, 0.2, decision="best")
