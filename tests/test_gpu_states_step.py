"""GPU tests (pytest -m gpu) of the by-word block step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_f32,
csrc/byword_step_states.inc) through the raw ctypes symbol.  Every comparison is exact.  The expected values come from the C oracle
alone (states_step_cases: oracle.vnet_decode for the decisions, the oracle's codec and calculate_states at memory log2 S for the
rest); tests/test_states_step_host.py shows on the CPU that the word sets reach every outcome of the codec."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as C
import meta_viterbinet_amd as mvn
import states_step_cases as SC
from meta_viterbinet_amd.trials import TrialBank
from step_call import SENTINEL, step

pytestmark = pytest.mark.gpu

ALL = ("dec", "msg", "enc", "lw", "labels", "nerr")
REQUESTS = [("nerr",), ("nerr", "labels"), ("msg", "nerr"), ("enc",), ("lw", "labels")]  # test_gpu_byword_codec.py's
NULL_IN_TURN = [tuple(n for n in ALL if n != out) for out in ALL]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


def _dev_weights(w, dev):
    return [torch.as_tensor(a).to(dev).contiguous() for a in w]


def _check(tag, out, row, ref, dec, names=ALL):
    """The requested outputs' rows equal the expected step's, and every padding element kept its sentinel."""
    expect = {"dec": dec, "msg": ref["msg"], "nerr": ref["nerr"], "enc": ref["enc"], "lw": ref["label_word"], "labels": ref["labels"]}
    for name in names:
        if name not in out or expect[name] is None:
            continue
        got = out[name] if name == "nerr" else out[name][:, :row[name]]
        if not np.array_equal(got, expect[name]):
            idx = np.argwhere(got != expect[name])
            pytest.fail(f"{tag}: {name}{idx[0].tolist()} = {got[tuple(idx[0])]}, expected {expect[name][tuple(idx[0])]}; "
                        f"{len(idx)} elements differ")
        if name != "nerr":
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{tag}: padding of {name} written"


# ------------------------------------------------------------------------------------------------------------- the word sets
@pytest.mark.parametrize("S", SC.STATES)
def test_word_set_in_one_launch(oracle, golden, dev, S):
    """All words of the set in one launch with one weight set: dec is mvn_vnet_decode_f32's and the oracle's, everything after it the
    oracle's step on that detection.  Then every word alone (R = 1)."""
    ws = SC.word_set(golden, S)
    dec, ref = SC.detected(golden, S)
    wd = _dev_weights(ws["w"], dev)
    out, row = SC.launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], wd)
    det = mvn.VNETDetector(S, {"train": SC.T_WORD, "val": SC.T_WORD}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), wd):
            p.copy_(a.reshape(p.shape))
        lib_dec = det(torch.as_tensor(ws["rx"]).to(dev), "val").cpu().numpy()
    assert np.array_equal(lib_dec, dec), "mvn_vnet_decode_f32 against the oracle"
    _check(f"S={S} R={dec.shape[0]}", out, row, ref, dec)
    for r in (0, int(np.flatnonzero(ref["nerr"] > 0)[0]), int(np.flatnonzero(ref["nerr"] == 0)[-1])):
        one, _ = SC.launch(dev, S, ws["rx"][r:r + 1], ws["msg"][r:r + 1], ws["nsym"], wd)
        for name in ALL:
            assert np.array_equal(one[name], out[name][r:r + 1]), (S, r, name)


def test_four_state_words_are_transmits(golden, dev):
    """The 4-state set's received words are mvn.transmit's for the same bits and noise draws (states_step_cases.isi_awgn)."""
    msg, cw, rx, noise = SC._s4_words()
    half = SC.S4_WORDS // 2
    h = mvn.estimate_channel(2, SC.GAMMA, "time_decay")
    for i, snr in enumerate(SC.S4_SNRS_DB):
        sel = slice(i * half, (i + 1) * half)
        y = mvn.transmit(torch.as_tensor(cw[sel]).to(dev), h, snr, 2, torch.as_tensor(noise[sel]).to(dev))
        assert np.array_equal(y.cpu().numpy(), rx[sel])


@pytest.mark.parametrize("S", SC.STATES)
def test_word_set_with_a_weight_set_per_word(oracle, golden, dev, S):
    """R weight sets through w_stride (a TrialBank's rows; the sets of rows >= 1 scaled by their own factor): word r is detected with
    set r, and its codec outputs follow from ITS detection."""
    ws = SC.word_set(golden, S)
    R = ws["rx"].shape[0]
    w = [[(a * np.float32(f)).astype(np.float32) for a in ws["w"]] for f in np.concatenate([[1.0], np.linspace(0.9, 1.1, R - 1)])]
    bank = TrialBank(w, S, SC.memory(S), dev)
    dec = np.concatenate([oracle.vnet_decode(ws["rx"][r:r + 1], w[r]) for r in range(R)])
    assert not np.array_equal(dec, SC.detected(golden, S)[0])  # the perturbed sets do decide differently
    ref = SC.expected_step(dec, ws["msg"], ws["nsym"], False, S)
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = SC.launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], wp, w_stride=[bank.P] * 6)
    _check(f"S={S} per-word weights", out, row, ref, dec)


# ------------------------------------------------------------------------------------------------------------- the smallest shapes
def _shapes(S):
    """(T, nsym): one tile; a half-empty last tile; a ragged last tile and more tiles than waves; the LDS bound (the round-robin wraps,
    at 1024 the codec's `p += 64` loops); the NS = 8 instantiation."""
    return [(16, 1), (24, 2), (136, 2), (mvn._lib.step_max_symbols(S), 2), (136, 8)]


@pytest.mark.parametrize("weights", ["random", "trained"])
@pytest.mark.parametrize("shape", range(5), ids=["one_tile", "half_tile", "ragged", "max_symbols", "nsym8"])
@pytest.mark.parametrize("S", SC.STATES)
def test_smallest_shapes(oracle, golden, dev, S, shape, weights):
    T, nsym = _shapes(S)[shape]
    case = SC.small_case(golden, S, T, nsym, weights)
    dec = oracle.vnet_decode(case["rx"], case["w"])
    ref = SC.expected_step(dec, case["msg"], nsym, False, S)
    out, row = SC.launch(dev, S, case["rx"], case["msg"], nsym, _dev_weights(case["w"], dev))
    _check(f"S={S} T={T} nsym={nsym} {weights}", out, row, ref, dec)
    if weights == "trained" and T >= 136:
        assert 0 < np.count_nonzero(dec != case["cw"]) < dec.size // 4  # some errors, not noise


@pytest.mark.parametrize("nsym", [2, 8])
@pytest.mark.parametrize("S", SC.STATES)
def test_pilot_step(oracle, golden, dev, S, nsym):
    """Pilot: enc = label word = the oracle's rs_encode(tx), nerr 0, labels with the word's own memory length; dec and msg untouched.
    rx is NULL: nothing is detected."""
    ws = SC.word_set(golden, S)
    tx = ws["msg"][:5, :SC.T_WORD - 8 * nsym]
    out, row = SC.launch(dev, S, None, tx, nsym, _dev_weights(ws["w"], dev), pilot=True)
    word = oracle.rs_encode_bits(tx, nsym)
    assert np.array_equal(out["enc"], word) and np.array_equal(out["lw"], word)
    assert np.array_equal(out["labels"], oracle.calculate_states(SC.memory(S), word).reshape(word.shape))
    assert not out["nerr"].any()
    assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])


# ------------------------------------------------------------------------------------- leading dimensions, optional outputs
@pytest.mark.parametrize("pilot", [False, True])
@pytest.mark.parametrize("S", [8, 128])
def test_step_honours_every_leading_dimension(oracle, golden, dev, S, pilot):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's."""
    ws = SC.word_set(golden, S)
    dec, ref = SC.detected(golden, S)
    T, K = SC.T_WORD, SC.T_WORD - 16
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6}
    out, row = SC.launch(dev, S, ws["rx"], ws["msg"], 2, _dev_weights(ws["w"], dev), pilot=pilot, ld=ld)
    if pilot:
        assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])
        _check(f"S={S} pilot ld", out, row, SC.expected_step(None, ws["msg"], 2, True, S), None, names=("nerr", "enc", "lw", "labels"))
    else:
        _check(f"S={S} ld", out, row, ref, dec)


@pytest.mark.parametrize("want", REQUESTS + NULL_IN_TURN, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("S", [8, 128])
def test_step_with_some_outputs_only(oracle, golden, dev, S, want):
    """Outputs not requested are NULL: test_gpu_byword_codec.py's five sets, and each output NULL in turn."""
    ws = SC.word_set(golden, S)
    dec, ref = SC.detected(golden, S)
    out, row = SC.launch(dev, S, ws["rx"], ws["msg"], 2, _dev_weights(ws["w"], dev), want=want)
    assert sorted(out) == sorted(want)
    _check(f"S={S} want={want}", out, row, ref, dec, names=want)


# ------------------------------------------------------------------------------------------------------------- torch.min's rule
@pytest.mark.parametrize("odd", ["nan_in_b3", "inf_in_W3"])
@pytest.mark.parametrize("S", SC.STATES)
def test_partly_odd_costs_follow_torch_min(oracle, golden, dev, S, odd):
    """A NaN in one entry of b3 / +inf in one row of W3: some but not all of a symbol's costs are NaN or infinite.  The decisions are
    the oracle's (torch.argmin: the first NaN is minimal; torch.min: NaN when either candidate is NaN)."""
    ws = SC.word_set(golden, S)
    w = [a.copy() for a in ws["w"]]
    if odd == "nan_in_b3":
        w[5][S // 2 + 1] = np.nan
    else:
        w[4][S // 2 - 1, :] = np.inf
    rx = ws["rx"][:8]
    dec, logits = oracle.vnet_decode(rx, w, want_logits=True)
    bad = ~np.isfinite(logits)
    assert bad.any(axis=2).all() and not bad.all(axis=2).any()  # every symbol: some costs odd, never all
    ref = SC.expected_step(dec, ws["msg"][:8], 2, False, S)
    out, row = SC.launch(dev, S, rx, ws["msg"][:8], 2, _dev_weights(w, dev))
    _check(f"S={S} {odd}", out, row, ref, dec)


# ------------------------------------------------------------------------------------------------------------- 16 states
def test_sixteen_states_equal_the_sixteen_state_step(oracle, golden, dev):
    """S = 16 through the new entry point is mvn_vnet_byword_step_f32, here on G7's first 50 words (a message per word: the decoded
    detection, every fifth with a flipped bit)."""
    g7 = golden("g7_by_word")
    w = _dev_weights(C.g7_weights(golden), dev)
    rx = np.ascontiguousarray(g7["time_decay_y"][:50], dtype=np.float32)
    tx = oracle.rs_decode_bits(np.ascontiguousarray(g7["time_decay_detected"][:50], dtype=np.float32), 2)
    tx[::5, 7] = 1 - tx[::5, 7]
    for pilot in (False, True):
        new, _ = SC.launch(dev, 16, rx, tx, 2, w, pilot=pilot)
        old, _ = step(dev, "running", "vnet", rx, tx, 2, pilot, weights=w)
        for name in ALL:
            assert np.array_equal(new[name], old[name]), (pilot, name)
    assert new["nerr"].sum() == 0 and (old["enc"] != SENTINEL["enc"]).all()
