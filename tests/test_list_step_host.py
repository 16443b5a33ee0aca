"""CPU only: the referee of the list step (tests/list_cases.py) checked against the oracle, the conditions its inputs have to meet,
and what of mvn_vnet_byword_step_list_f32 / mvn_va_byword_step_list_f32 and decision='list' can be tested without a device.

  * sign(delta) is the oracle's traced-back word wherever delta != 0; erasure_fill returns the sent codeword when exactly the
    corrupted bytes (padded with clean ones) are erased.
  * On path_cases.words(136, 2, 64, snr), both detectors, m = 4: the list fails on strictly fewer words than the path, on no word the
    path decodes, picks a candidate other than the hard decoder's on at least 5 words, and no two different messages tie in metric.
    tests/test_gpu_list_step.py asserts the GPU's outputs on the same batches equal the referee's, so these carry over.
  * Keyword validation.  (Argument validation of both entry points: tests/test_step_validation_host.py.)"""
import re

import numpy as np
import pytest

import codec_cases as C
import list_cases as Lc
import meta_viterbinet_amd as mvn
import path_cases as P
from test_kernel_resources import resources  # noqa: F401  (the fixture that reads the built library's code object)

M_HOST = 4


@pytest.fixture(scope="module")
def batches(oracle, golden):
    w = C.g7_weights(golden)
    out = {}
    for snr in P.SNRS:
        msg, cw, y = P.words(P.T_HOST, P.NSYM_HOST, P.R_HOST, snr)
        for kind in P.KINDS:
            out[snr, kind] = dict(lst=Lc.expected(kind, y, msg, P.NSYM_HOST, M_HOST, weights=w),
                                  path=P.expected(kind, y, msg, P.NSYM_HOST, weights=w), cw=cw, msg=msg)
    return out


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_sign_of_delta_is_the_traced_back_word(batches, snr, kind):
    e = batches[snr, kind]["lst"]
    nz = e["delta"] != 0
    assert nz.mean() > 0.99
    assert np.array_equal((e["delta"] < 0)[nz], e["dec"][nz] == 1)
    assert np.array_equal(e["dec"], batches[snr, kind]["path"]["dec"])


def test_erasure_fill_returns_the_sent_codeword(oracle):
    """Every word of codec_cases' batches with at most nsym corrupted bytes (n <= 64): erase exactly those bytes, padded to nsym with
    clean ones."""
    words = 0
    for nsym, n in C.CASES:
        if n > 64:
            continue
        b = C.batch(nsym, n)
        for r, pos in enumerate(b["pos"]):
            if len(pos) > nsym:
                continue
            pad = [p for p in range(n - 1, -1, -1) if p not in pos][: nsym - len(pos)]
            got = Lc.erasure_fill(b["word"][r], list(pos) + pad, nsym)
            assert np.array_equal(got, b["cw"][r]), (nsym, n, r, pos)
            words += 1
    assert words >= 400, words


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_list_fails_less_than_the_path_and_never_where_it_decodes(batches, snr, kind):
    b = batches[snr, kind]
    lst, path = b["lst"], b["path"]
    failed_list, failed_path = lst["nerr"] > 0, path["nerr"] > 0
    moved = int((lst["choice"] != 0).sum())
    print(f"{snr} dB {kind}: failed words path {int(failed_path.sum())}, list {int(failed_list.sum())}; choice != 0 on {moved} words")
    assert int(failed_list.sum()) < int(failed_path.sum())
    assert not np.any(failed_list & ~failed_path)
    assert moved >= 5


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("snr", P.SNRS)
def test_no_two_different_messages_tie_in_metric(batches, snr, kind):
    e = batches[snr, kind]["lst"]
    K = P.T_HOST - 8 * P.NSYM_HOST
    for r in range(P.R_HOST):
        M, cands = e["metrics"][r], e["candidates"][r]
        for a in range(len(M)):
            for c in range(a + 1, len(M)):
                if M[a] == M[c]:
                    assert np.array_equal(cands[a][:K], cands[c][:K]), (r, a, c)


def test_list_step_kernels_resources(resources):  # noqa: F811
    """No scratch; the ViterbiNet form keeps to the 128 VGPRs of a 16-wave workgroup; the static LDS leaves room for the 64 KB of
    costs and forward metrics at T = 512 within the CU's 160 KB."""
    for pattern, budget in ((r"byword_list_step_kernel<(2|8)>", 128), (r"byword_list_step_va_kernel<(2|8)>", None)):
        names = [n for n in resources if re.fullmatch(pattern, n)]
        assert len(names) == 2, f"{pattern}: {names}"
        for n in names:
            print(n, resources[n])
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            if budget is not None:
                assert resources[n]["vgpr"] <= budget, f"{n}: {resources[n]['vgpr']} VGPRs, built for <= {budget}"
            assert resources[n]["lds"] + 64 * 1024 <= 160 * 1024, n


def test_list_keyword_is_validated():
    import torch

    from meta_viterbinet_amd.lstm import LSTMDetector
    from meta_viterbinet_amd.lstm_trials import LSTMTrialBank

    det = mvn.VNETDetector(16, {"train": 136, "val": 136})
    tx, rx = torch.zeros(2, 120), torch.zeros(2, 136)
    with pytest.raises(ValueError, match="decision"):
        mvn.eval_by_word(LSTMDetector(), tx, rx, 8.0, 0.2, 2, 4, decision="list")
    for bad in (1, 18, 12):  # below nsym, above the word's bytes, 66 erasure patterns
        with pytest.raises(ValueError, match="list_bytes"):
            mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="list", list_bytes=bad)
    with pytest.raises(ValueError, match="list_bytes"):
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="path", list_bytes=4)
    with pytest.raises(ValueError, match="512"):
        mvn.eval_by_word(mvn.VNETDetector(16, {"train": 520, "val": 520}), torch.zeros(2, 504), torch.zeros(2, 520), 8.0, 0.2, 2, 4,
                         decision="list")
    with pytest.raises(ValueError, match="fused_step"):
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="list", fused_step=False)
    with pytest.raises(ValueError, match="ROCm"):  # words on the CPU: no other route to fall back to
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="list")
    for fn in (mvn.eval_counters, mvn.single_eval_at_point, mvn.sharded_eval):
        with pytest.raises(ValueError, match="list_decode"):
            fn(det, tx, rx, 8.0, 0.2, decision="list")
    with pytest.raises(ValueError, match="list_decode"):
        mvn.list_decode(LSTMDetector(), rx, 2)
    with pytest.raises(ValueError, match="list_bytes"):
        mvn.list_decode(det, rx, 2, list_bytes=12)
    va = mvn.VADetector(16, C.L, 136, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    with pytest.raises(ValueError, match="gamma"):
        mvn.list_decode(va, rx, 2)
    bank = LSTMTrialBank.__new__(LSTMTrialBank)  # (the keyword is checked before the bank is looked into)
    with pytest.raises(ValueError, match="decision"):
        mvn.eval_by_word_batched(bank, tx.reshape(1, 2, 120), rx.reshape(1, 2, 136), 2, 4, [None], decision="list")
