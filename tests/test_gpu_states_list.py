"""GPU tests (pytest -m gpu) of the by-word LIST step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_list_f32,
csrc/byword_list_states.inc) through the raw ctypes symbol, of mvn.list_decode and of the two evaluations that take it
(harness.eval_by_word, trials.eval_by_word_batched with decision='list').  Every comparison with the referee is exact, delta included
(np.array_equal: -0 equals +0).  The expected values come from states_list_cases.expected -- the plain definition in NumPy fp32 over
the C oracle's logits, path and codec; tests/test_states_list_host.py shows on the CPU what the word sets put in front of the kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

import codec_cases as C
import meta_viterbinet_amd as mvn
import states_list_cases as LS
import states_path_cases as PC
import states_step_cases as SC
from meta_viterbinet_amd.trials import TrialBank, TrialDraws, eval_by_word_batched
from step_call import SENTINEL, step
from test_gpu_maml_states_trials import OWN, _alone_run, _assert_rows, _g21, _refuse_sequential
from test_gpu_states_path import _detector, _dev_weights, _flow

pytestmark = pytest.mark.gpu

ALL = LS.OUTPUTS
FLAT = ("nerr", "choice")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


def _check(tag, out, row, ref, names=ALL, rows=slice(None)):
    """The requested outputs' rows equal the referee's, and every padding element kept its sentinel."""
    for name in names:
        want = ref[name][rows]
        got = out[name] if name in FLAT else out[name][:, :row[name]]
        if not np.array_equal(got, want):
            idx = np.argwhere(got != want)
            pytest.fail(f"{tag}: {name}{idx[0].tolist()} = {got[tuple(idx[0])]}, expected {want[tuple(idx[0])]}; {len(idx)} elements differ")
        if name not in FLAT:
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{tag}: padding of {name} written"


# ------------------------------------------------------------------------------------------------------------- the word sets
@pytest.mark.parametrize("S", SC.STATES)
def test_word_set_in_one_launch(oracle, golden, dev, S):
    """All words of the set in one launch with one weight set, (nsym, m) = (2, 4): every output is the referee's; dec is also what the
    path states step returns for the same words.  Then three words alone (R = 1)."""
    ws = PC.word_set(golden, S)
    ref = LS.expected_set(golden, S)
    wd = _dev_weights(ws["w"], dev)
    out, row = LS.launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], 4, wd)
    _check(f"S={S} R={ws['rx'].shape[0]}", out, row, ref)
    path, _ = SC.launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], wd, entry=PC.ENTRY)
    assert np.array_equal(out["dec"], path["dec"])
    assert (out["choice"] != 0).sum() >= 2 and (out["nerr"] > 0).sum() < (path["nerr"] > 0).sum()
    for r in (0, int(np.flatnonzero(ref["choice"] != 0)[0]), int(np.flatnonzero(ref["nerr"] == 0)[-1])):
        one, _ = LS.launch(dev, S, ws["rx"][r:r + 1], ws["msg"][r:r + 1], ws["nsym"], 4, wd)
        for name in ALL:
            assert np.array_equal(one[name], out[name][r:r + 1]), (S, r, name)


# ------------------------------------------------------------------------------------------------------------- the small cases
COMBOS = [(1, 3), (2, 4), (2, 8), (3, 6), (8, 9)]  # 3, 6, 28, 20 and 9 candidates; (8, 9): the NS = 8 instantiation
LENGTHS = ["shortest", "t24", "t136", "max_symbols"]


def _small_shapes(S, length):
    """(T, nsym, m) of one length kind, where T allows the pair (m <= T / 8 bytes, T / 8 > nsym): the shortest legal word of each nsym,
    a word shorter than one 32-stage block of the walk, the reference's word, the LDS bound."""
    if length == "shortest":
        shapes = [(8 * (nsym + 1), nsym, m) for nsym, m in COMBOS] + [(16, 1, 2)]
    else:
        T = {"t24": 24, "t136": 136, "max_symbols": mvn._lib.list_max_symbols(S)}[length]
        shapes = [(T, nsym, m) for nsym, m in COMBOS]
    return [(T, nsym, m) for T, nsym, m in shapes if nsym < T // 8 and m <= T // 8]


@pytest.mark.parametrize("weights", ["random", "trained"])
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("S", SC.STATES)
def test_small_cases(oracle, golden, dev, S, length, weights):
    """Six words per shape through the referee once; R = 1 and R = 5 of them through the kernel."""
    shapes = _small_shapes(S, length)
    assert shapes and (length in ("shortest", "t24") or len(shapes) == len(COMBOS))
    for T, nsym, m in shapes:
        case = SC.small_case(golden, S, T, nsym, weights)
        ref = LS.expected(case, m)
        assert ref["candidates"].shape[1] == 1 + math.comb(m, nsym)
        wd = _dev_weights(case["w"], dev)
        for R in (1, 5):
            out, row = LS.launch(dev, S, case["rx"][:R], case["msg"][:R], nsym, m, wd)
            _check(f"S={S} T={T} nsym={nsym} m={m} R={R} {weights}", out, row, ref, rows=slice(0, R))


# ------------------------------------------------------------------------------------------------------------- call variants
@pytest.mark.parametrize("S", SC.STATES)
def test_word_set_with_a_weight_set_per_word(oracle, golden, dev, S):
    """R weight sets through w_stride (a TrialBank's rows; the sets of rows >= 1 scaled by their own factor), 12 words."""
    ws = PC.word_set(golden, S)
    R = 12
    case = dict(ws, rx=ws["rx"][:R], msg=ws["msg"][:R])
    w = [[(a * np.float32(f)).astype(np.float32) for a in ws["w"]] for f in np.concatenate([[1.0], np.linspace(0.9, 1.1, R - 1)])]
    ref = LS.expected(case, 4, w=w)
    assert not np.array_equal(ref["delta"], LS.expected_set(golden, S)["delta"][:R])
    bank = TrialBank(w, S, SC.memory(S), dev)
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = LS.launch(dev, S, case["rx"], case["msg"], 2, 4, wp, w_stride=[bank.P] * 6)
    _check(f"S={S} per-word weights", out, row, ref)


@pytest.mark.parametrize("S", [8, 128])
def test_step_honours_every_leading_dimension(oracle, golden, dev, S):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's."""
    ws = PC.word_set(golden, S)
    T, K = SC.T_WORD, SC.T_WORD - 16
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6, "delta": T + 9}
    out, row = LS.launch(dev, S, ws["rx"], ws["msg"], 2, 4, _dev_weights(ws["w"], dev), ld=ld)
    _check(f"S={S} ld", out, row, LS.expected_set(golden, S))


REQUESTS = [("nerr",), ("nerr", "labels"), ("msg", "nerr"), ("enc",), ("lw", "labels"), ("delta",), ("choice", "nerr"),
            ("dec", "delta", "choice", "msg")]
NULL_IN_TURN = [tuple(n for n in ALL if n != out) for out in ALL]
NO_TX = [("msg", "dec", "delta", "choice"), ("msg",), ("enc", "choice")]


@pytest.mark.parametrize("want", REQUESTS + NULL_IN_TURN, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("S", [8, 128])
def test_step_with_some_outputs_only(oracle, golden, dev, S, want):
    """Outputs not requested are NULL."""
    ws = PC.word_set(golden, S)
    out, row = LS.launch(dev, S, ws["rx"], ws["msg"], 2, 4, _dev_weights(ws["w"], dev), want=want)
    assert sorted(out) == sorted(want)
    _check(f"S={S} want={want}", out, row, LS.expected_set(golden, S), names=want)


@pytest.mark.parametrize("want", NO_TX, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("S", SC.STATES)
def test_step_without_a_transmitted_word(oracle, golden, dev, S, want):
    """tx = NULL on a data step when nerr, label_word and labels are NULL: a decoder without a genie."""
    ws = PC.word_set(golden, S)
    out, row = LS.launch(dev, S, ws["rx"], None, 2, 4, _dev_weights(ws["w"], dev), want=want)
    _check(f"S={S} no tx want={want}", out, row, LS.expected_set(golden, S), names=want)


@pytest.mark.parametrize("nsym,m", [(2, 4), (8, 9)])
@pytest.mark.parametrize("S", SC.STATES)
def test_pilot_through_the_list_entry_is_the_running_pilot(oracle, golden, dev, S, nsym, m):
    """A pilot detects nothing: every output is what mvn_vnet_byword_step_states_f32's pilot step writes (rx NULL); delta and choice
    keep their sentinels."""
    ws = PC.word_set(golden, S)
    tx = ws["msg"][:5, :SC.T_WORD - 8 * nsym]
    wd = _dev_weights(ws["w"], dev)
    out, row = LS.launch(dev, S, None, tx, nsym, m, wd, pilot=True)
    old, _ = SC.launch(dev, S, None, tx, nsym, wd, pilot=True)
    for name in old:
        assert np.array_equal(out[name], old[name]), name
    word = oracle.rs_encode_bits(tx, nsym)
    assert np.array_equal(out["enc"], word) and np.array_equal(out["lw"], word) and not out["nerr"].any()
    assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])
    assert np.all(out["delta"] == SENTINEL["delta"]) and np.all(out["choice"] == SENTINEL["choice"])


def test_sixteen_states_equal_the_sixteen_state_list_step(oracle, golden, dev):
    """S = 16 through the new entry point is mvn_vnet_byword_step_list_f32, here on G7's first 50 words (a message per word: the decoded
    detection, every fifth with a flipped bit)."""
    g7 = golden("g7_by_word")
    w = _dev_weights(C.g7_weights(golden), dev)
    rx = np.ascontiguousarray(g7["time_decay_y"][:50], dtype=np.float32)
    tx = oracle.rs_decode_bits(np.ascontiguousarray(g7["time_decay_detected"][:50], dtype=np.float32), 2)
    tx[::5, 7] = 1 - tx[::5, 7]
    for pilot in (False, True):
        new, _ = LS.launch(dev, 16, rx, tx, 2, 4, w, pilot=pilot)
        old, _ = step(dev, "list", "vnet", rx, tx, 2, pilot, m=4, weights=w)
        assert sorted(new) == sorted(old)
        for name in ALL:
            assert np.array_equal(new[name], old[name], equal_nan=True), (pilot, name)
    assert (new["choice"] == SENTINEL["choice"]).all() and not (new["enc"] == SENTINEL["enc"]).any()


# ------------------------------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize("odd", ["nan_weight", "inf_sample"])
@pytest.mark.parametrize("S", SC.STATES)
def test_non_finite_inputs_stay_in_range(oracle, golden, dev, S, odd):
    """A NaN in one entry of b3 / a +inf and a -inf sample in every word: dec is the path step's, choice lies in [0, C(m, nsym)] and
    every output was written.  Nothing more is specified."""
    ws = PC.word_set(golden, S)
    w = [a.copy() for a in ws["w"]]
    rx = ws["rx"][:8].copy()
    if odd == "nan_weight":
        w[5][S // 2 + 1] = np.nan
    else:
        rx[:, 17] = np.inf
        rx[:, 90] = -np.inf
    if odd == "nan_weight":  # (the sigmoid layer may well map an infinite sample to finite logits: the case is about the sample)
        assert not np.all(np.isfinite(oracle.vnet_logits(rx, w)))
    wd = _dev_weights(w, dev)
    out, row = LS.launch(dev, S, rx, ws["msg"][:8], 2, 4, wd)
    path, _ = SC.launch(dev, S, rx, ws["msg"][:8], 2, wd, entry=PC.ENTRY)
    assert np.array_equal(out["dec"], path["dec"])
    if odd == "nan_weight":
        assert np.array_equal(out["dec"], PC.path(rx, w))
    assert np.all((out["choice"] >= 0) & (out["choice"] <= math.comb(4, 2)))
    for name in ALL:
        got = out[name] if name in FLAT else out[name][:, :row[name]]
        assert not np.any(got == SENTINEL[name]), f"{name} not written"
    assert np.all((out["labels"] >= 0) & (out["labels"] < S)) and np.all((out["nerr"] >= 0) & (out["nerr"] <= 120))
    for name in ("msg", "enc", "lw"):
        assert np.all((out[name] == 0) | (out[name] == 1)), name
    again, _ = LS.launch(dev, S, rx, ws["msg"][:8], 2, 4, wd)
    for name in ALL:
        assert np.array_equal(again[name], out[name], equal_nan=True), f"{name} differs between two launches"


# ------------------------------------------------------------------------------------------------------------- list_decode
@pytest.mark.parametrize("S", [8, 64])
def test_list_decode_is_the_step_without_a_genie(oracle, golden, dev, S):
    ws = PC.word_set(golden, S)
    ref = LS.expected_set(golden, S)
    det = _detector(ws["w"], S, SC.T_WORD, dev)
    msg, choice, delta = mvn.list_decode(det, torch.as_tensor(ws["rx"]).to(dev), 2, return_delta=True)
    assert np.array_equal(msg.cpu().numpy(), ref["msg"]) and np.array_equal(delta.cpu().numpy(), ref["delta"])
    assert np.array_equal(choice.cpu().numpy(), ref["choice"])
    two = mvn.list_decode(det, torch.as_tensor(ws["rx"]).to(dev), 2, list_bytes=4)
    assert len(two) == 2 and torch.equal(two[0], msg) and torch.equal(two[1], choice)  # the default m is n_symbols + 2


# ------------------------------------------------------------------------------------------------------------- the flows
@pytest.mark.parametrize("S", [8, 128])
def test_eval_by_word_list_without_updates(oracle, golden, dev, S):
    """harness.eval_by_word(decision='list') without updates on the word set: ser_by_word is the referee's nerr over K in the
    reference's arithmetic (block 0 is a pilot: 0)."""
    ws = PC.word_set(golden, S)
    ref = LS.expected_set(golden, S)
    N, K = ws["msg"].shape
    det = _detector(ws["w"], S, SC.T_WORD, dev)
    ser = mvn.eval_by_word(det, torch.as_tensor(ws["msg"]).to(dev), torch.as_tensor(ws["rx"]).to(dev), 9.0, 0.2, 2, N + 1, decision="list")
    want = mvn.metrics.ser_from_errors(ref["nerr"], K)
    want[0] = 0.0
    assert np.array_equal(ser, want)
    assert np.allclose(ser, np.where(np.arange(N) > 0, ref["nerr"] / K, 0.0), rtol=0, atol=1e-7) and (ser > 0).sum() >= (0 if S == 8 else 2)


def _sequential(tx, rx, w0, S, nsym, sub, kw, draws, dev):
    det = _detector(w0, S, rx.shape[1], dev)
    tr = mvn.OnlineTrainer(det, SC.memory(S))
    ser = mvn.eval_by_word(det, tx, rx, 9.0, 0.2, nsym, sub, online_trainer=tr, draws=draws(), decision="list", **kw)
    return ser, [p.detach().clone() for p in det.parameters()], tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step


@pytest.mark.parametrize("S", [8, 64])
def test_batched_list_trials_equal_sequential_runs(golden, dev, monkeypatch, S):
    """G16 L3_selfsup / G17 L6_selfsup, recorded draws, 8 iterations: trials.eval_by_word_batched(decision='list') with 3 trials equals
    three harness.eval_by_word(decision='list') runs -- rows, error counts, final weights and optimizer state -- with one launch of the
    list states step per block for all trials."""
    R = 3
    tx, rx, w0, nsym, sub, kw, draws = _flow(golden, S, dev, R)
    seq = [_sequential(tx[r], rx[r], w0, S, nsym, sub, kw, draws, dev) for r in range(R)]
    lib = mvn._lib.load()
    calls = {"step": 0}
    step_fn = getattr(lib, LS.ENTRY)

    def counted(*a):
        calls["step"] += 1
        return step_fn(*a)

    monkeypatch.setattr(lib, LS.ENTRY, counted)
    bank = TrialBank([w0] * R, S, SC.memory(S), dev)
    record = {}
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, [draws() for _ in range(R)], decision="list", record=record, **kw)
    assert calls["step"] == tx.shape[1]
    K = tx.shape[2]
    for r, (ser, wr, m, v, n) in enumerate(seq):
        assert np.array_equal(ser, ser_b[r]), (r, np.flatnonzero(ser != ser_b[r]))
        assert np.array_equal(mvn.metrics.ser_from_errors(record["nerr"][r], K), ser), r
        for a, b in zip(wr, bank.weights(r)):
            assert torch.equal(a, b), r
        assert torch.equal(m, bank.exp_avg[r]) and torch.equal(v, bank.exp_avg_sq[r]) and n == int(bank.step[r]) and n > 0, r
    assert len({tuple(row) for row in ser_b}) > 1  # the trials are not copies of each other


def test_list_trials_with_meta_learning_go_lock_step(golden, dev, monkeypatch):
    """online_meta at 64 states, where decision='path' takes the lock-step engine through _meta_states_serves: so does decision='list'.
    R = 3 over the first 16 blocks of G21's flow; each row is harness.eval_by_word(decision='list') alone on that trial."""
    S, R = 64, 3
    g, tag, w0, tx, rx, nsym, sub, kw = _g21(golden, S, dev, 16, R)
    kw.update(OWN, decision="list")
    rows = [_alone_run(S, w0, tx[r], rx[r], nsym, sub, TrialDraws(500 + r, dev), dev, kw) for r in range(R)]
    _refuse_sequential(monkeypatch)
    bank = TrialBank([w0] * R, S, SC.memory(S), dev)
    rec = {}
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, [TrialDraws(500 + r, dev) for r in range(R)], record=rec, **kw)
    _assert_rows(bank, ser_b, rec, rows)
    assert rec["meta"][0].any() and len({tuple(row) for row in ser_b}) > 1
