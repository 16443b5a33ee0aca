"""GPU tests (pytest -m gpu) of the by-word PATH step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_path_f32,
csrc/byword_step_states.inc) through the raw ctypes symbol, and of the two evaluations that take it (harness.eval_by_word,
trials.eval_by_word_batched with decision='path').  Every comparison is exact.  The expected values of the step come from the C oracle
alone (states_path_cases.path: vnet_logits -> acs_sweep_surv -> traceback; then the oracle's codec and calculate_states at memory
log2 S); tests/test_states_path_host.py shows on the CPU that the word sets reach every outcome of the codec under the path."""
import ctypes

import numpy as np
import pytest
import torch

import codec_cases as C
import meta_viterbinet_amd as mvn
import states_path_cases as PC
import states_step_cases as SC
from meta_viterbinet_amd.trials import TrialBank, eval_by_word_batched
from step_call import SENTINEL, step
from test_gpu_reference_flow import RecordedTableDraws, _flow_kwargs

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


def _launch(dev, S, rx, tx, nsym, w, **kw):
    return SC.launch(dev, S, rx, tx, nsym, w, entry=PC.ENTRY, **kw)


def _detector(w, S, T, dev):
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w):
            p.copy_(torch.as_tensor(a).reshape(p.shape))
    return det


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
    """All words of the set in one launch with one weight set: dec is the oracle's path and VNETDetector.viterbi_path's, everything
    after it the oracle's step on that path.  Then three words alone (R = 1)."""
    ws = PC.word_set(golden, S)
    dec, running, ref = PC.detected(golden, S)
    wd = _dev_weights(ws["w"], dev)
    out, row = _launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], wd)
    det = _detector(ws["w"], S, SC.T_WORD, dev)
    with torch.no_grad():
        lib_dec = det.viterbi_path(torch.as_tensor(ws["rx"]).to(dev)).cpu().numpy()
    assert np.array_equal(lib_dec, dec), "VNETDetector.viterbi_path against the oracle"
    _check(f"S={S} R={dec.shape[0]}", out, row, ref, dec)
    assert not np.array_equal(out["dec"], running)
    for r in (0, int(np.flatnonzero(ref["nerr"] > 0)[0]), int(np.flatnonzero(ref["nerr"] == 0)[-1])):
        one, _ = _launch(dev, S, ws["rx"][r:r + 1], ws["msg"][r:r + 1], ws["nsym"], wd)
        for name in ALL:
            assert np.array_equal(one[name], out[name][r:r + 1]), (S, r, name)


@pytest.mark.parametrize("S", SC.STATES)
def test_word_set_with_a_weight_set_per_word(oracle, golden, dev, S):
    """R weight sets through w_stride (a TrialBank's rows; the sets of rows >= 1 scaled by their own factor): word r is detected with
    set r, and its codec outputs follow from ITS path."""
    ws = PC.word_set(golden, S)
    R = ws["rx"].shape[0]
    w = [[(a * np.float32(f)).astype(np.float32) for a in ws["w"]] for f in np.concatenate([[1.0], np.linspace(0.9, 1.1, R - 1)])]
    bank = TrialBank(w, S, SC.memory(S), dev)
    dec = np.concatenate([PC.path(ws["rx"][r:r + 1], w[r]) for r in range(R)])
    assert not np.array_equal(dec, PC.detected(golden, S)[0])  # the perturbed sets do decide differently
    ref = SC.expected_step(dec, ws["msg"], ws["nsym"], False, S)
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = _launch(dev, S, ws["rx"], ws["msg"], ws["nsym"], wp, w_stride=[bank.P] * 6)
    _check(f"S={S} per-word weights", out, row, ref, dec)


# ------------------------------------------------------------------------------------------------------------- the smallest shapes
def _shapes(S):
    """(T, nsym): one tile; a half-empty last tile; a ragged last tile, more tiles than waves and a walk whose lowest 32 stages start
    below 0; the LDS bound (the walk's fetch-ahead runs its whole length); the NS = 8 instantiation.  (T = 8, fewer stages than a
    fetch: the check admits no such word, T / 8 > nsym >= 1.)"""
    return [(16, 1), (24, 2), (136, 2), (mvn._lib.step_max_symbols(S), 2), (136, 8)]


@pytest.mark.parametrize("weights", ["random", "trained"])
@pytest.mark.parametrize("shape", range(5), ids=["one_tile", "half_tile", "ragged", "max_symbols", "nsym8"])
@pytest.mark.parametrize("S", SC.STATES)
def test_smallest_shapes(oracle, golden, dev, S, shape, weights):
    T, nsym = _shapes(S)[shape]
    case = SC.small_case(golden, S, T, nsym, weights)
    dec = PC.path(case["rx"], case["w"])
    ref = SC.expected_step(dec, case["msg"], nsym, False, S)
    out, row = _launch(dev, S, case["rx"], case["msg"], nsym, _dev_weights(case["w"], dev))
    _check(f"S={S} T={T} nsym={nsym} {weights}", out, row, ref, dec)


@pytest.mark.parametrize("nsym", [2, 8])
@pytest.mark.parametrize("S", SC.STATES)
def test_pilot_through_the_path_entry_is_the_running_pilot(oracle, golden, dev, S, nsym):
    """A pilot detects nothing: every output is what mvn_vnet_byword_step_states_f32's pilot step writes (rx NULL)."""
    ws = PC.word_set(golden, S)
    tx = ws["msg"][:5, :SC.T_WORD - 8 * nsym]
    wd = _dev_weights(ws["w"], dev)
    out, row = _launch(dev, S, None, tx, nsym, wd, pilot=True)
    old, _ = SC.launch(dev, S, None, tx, nsym, wd, pilot=True)
    for name in ALL:
        assert np.array_equal(out[name], old[name]), name
    word = oracle.rs_encode_bits(tx, nsym)
    assert np.array_equal(out["enc"], word) and np.array_equal(out["lw"], word) and not out["nerr"].any()
    assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])


# ------------------------------------------------------------------------------------- leading dimensions, optional outputs
@pytest.mark.parametrize("S", [8, 128])
def test_step_honours_every_leading_dimension(oracle, golden, dev, S):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's."""
    ws = PC.word_set(golden, S)
    dec, _, ref = PC.detected(golden, S)
    T, K = SC.T_WORD, SC.T_WORD - 16
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6}
    out, row = _launch(dev, S, ws["rx"], ws["msg"], 2, _dev_weights(ws["w"], dev), ld=ld)
    _check(f"S={S} ld", out, row, ref, dec)


@pytest.mark.parametrize("want", REQUESTS + NULL_IN_TURN, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("S", [8, 128])
def test_step_with_some_outputs_only(oracle, golden, dev, S, want):
    """Outputs not requested are NULL: test_gpu_byword_codec.py's five sets, and each output NULL in turn."""
    ws = PC.word_set(golden, S)
    dec, _, ref = PC.detected(golden, S)
    out, row = _launch(dev, S, ws["rx"], ws["msg"], 2, _dev_weights(ws["w"], dev), want=want)
    assert sorted(out) == sorted(want)
    _check(f"S={S} want={want}", out, row, ref, dec, names=want)


# ------------------------------------------------------------------------------------------------------------- torch.min's rule
@pytest.mark.parametrize("odd", ["nan_in_b3", "inf_in_W3", "all_ties"])
@pytest.mark.parametrize("S", SC.STATES)
def test_survivors_and_argmin_follow_torch(oracle, golden, dev, S, odd):
    """A NaN in one entry of b3 / +inf in one row of W3: some but not all of a symbol's costs are NaN or infinite (torch.min: the first
    NaN, torch.argmin: a NaN minimal).  W3 = 0, b3 = 0: every ACS is a tie, every survivor bit 0, the argmin state 0, the path all
    zeros.  The path is the oracle's."""
    ws = PC.word_set(golden, S)
    w = [a.copy() for a in ws["w"]]
    if odd == "nan_in_b3":
        w[5][S // 2 + 1] = np.nan
    elif odd == "inf_in_W3":
        w[4][S // 2 - 1, :] = np.inf
    else:
        w[4][:] = 0.0
        w[5][:] = 0.0
    rx = ws["rx"][:8]
    logits = oracle.vnet_logits(rx, w)
    bad = ~np.isfinite(logits)
    dec = PC.path(rx, w)
    if odd == "all_ties":
        assert not logits.any() and not dec.any()
    else:
        assert bad.any(axis=2).all() and not bad.all(axis=2).any()  # every symbol: some costs odd, never all
    ref = SC.expected_step(dec, ws["msg"][:8], 2, False, S)
    out, row = _launch(dev, S, rx, ws["msg"][:8], 2, _dev_weights(w, dev))
    _check(f"S={S} {odd}", out, row, ref, dec)


# ------------------------------------------------------------------------------------------------------------- 16 states
def test_sixteen_states_equal_the_sixteen_state_path_step(oracle, golden, dev):
    """S = 16 through the new entry point is mvn_vnet_byword_step_path_f32, here on G7's first 50 words (a message per word: the decoded
    detection, every fifth with a flipped bit)."""
    g7 = golden("g7_by_word")
    w = _dev_weights(C.g7_weights(golden), dev)
    rx = np.ascontiguousarray(g7["time_decay_y"][:50], dtype=np.float32)
    tx = oracle.rs_decode_bits(np.ascontiguousarray(g7["time_decay_detected"][:50], dtype=np.float32), 2)
    tx[::5, 7] = 1 - tx[::5, 7]
    for pilot in (False, True):
        new, _ = _launch(dev, 16, rx, tx, 2, w, pilot=pilot)
        old, _ = step(dev, "path", "vnet", rx, tx, 2, pilot, weights=w)
        for name in ALL:
            assert np.array_equal(new[name], old[name]), (pilot, name)


# ------------------------------------------------------------------------------------------------------------- the flows
def _flow(golden, S, dev, n_trials=1):
    """The self-supervised flow of golden G16 / G17 at S states: its 50 blocks, its iteration count and its recorded minibatches
    (where the path trains on a block the reference did not: the table's valid filler).  n_trials > 1: the golden's words and copies
    with fresh noise on rx."""
    name, tag = SC.FLOW[S]
    g = golden(name)
    kw, opt, nsym, sub = _flow_kwargs(g, None, tag, dev)
    assert not opt and kw["self_supervised_iterations"] == 8 and not kw.get("online_meta")
    tx1 = torch.tensor(g[f"{tag}_tx"], device=dev).float()
    rx1 = torch.tensor(g[f"{tag}_rx"], device=dev)
    assert tx1.shape[0] == 50
    gen = torch.Generator(device=dev).manual_seed(128 + S)
    rx = torch.stack([rx1] + [rx1 + 0.15 * torch.randn(rx1.shape, generator=gen, device=dev) for _ in range(n_trials - 1)]).contiguous()
    tx = tx1.unsqueeze(0).repeat(n_trials, 1, 1).contiguous()
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]

    def draws():
        return RecordedTableDraws(g, tag, 8, sub, dev, lenient=True)

    return tx, rx, w0, nsym, sub, kw, draws


def _spy(monkeypatch):
    """Counts the calls of the path states step and of the separate launches' detector on the loaded library."""
    lib = mvn._lib.load()
    calls = {"step": 0, "surv": 0}
    step_fn, surv_fn = getattr(lib, PC.ENTRY), lib.mvn_vnet_decode_surv_f32

    def counted_step(*a):
        calls["step"] += 1
        return step_fn(*a)

    def counted_surv(*a):
        calls["surv"] += 1
        return surv_fn(*a)

    monkeypatch.setattr(lib, PC.ENTRY, counted_step)
    monkeypatch.setattr(lib, "mvn_vnet_decode_surv_f32", counted_surv)
    return calls


def _sequential(tx, rx, w0, S, nsym, sub, kw, draws, dev, **more):
    det = _detector(w0, S, rx.shape[1], dev)
    tr = mvn.OnlineTrainer(det, SC.memory(S))
    ser = mvn.eval_by_word(det, tx, rx, 9.0, 0.2, nsym, sub, online_trainer=tr, draws=draws(), decision="path", **more, **kw)
    return ser, [p.detach().clone() for p in det.parameters()], tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step


@pytest.mark.parametrize("S", [8, 64])
def test_eval_by_word_path_takes_one_launch_per_block(golden, dev, monkeypatch, S):
    """harness.eval_by_word(decision='path') on the 50 blocks of the flow: ser_by_word, final weights, both moments and the step count
    equal the separate launches' (fused_step=False); the path states step ran once per block, mvn_vnet_decode_surv_f32 never."""
    tx, rx, w0, nsym, sub, kw, draws = _flow(golden, S, dev)
    calls = _spy(monkeypatch)
    want = _sequential(tx[0], rx[0], w0, S, nsym, sub, kw, draws, dev, fused_step=False)
    assert calls["step"] == 0 and calls["surv"] == 50
    calls["surv"] = 0
    got = _sequential(tx[0], rx[0], w0, S, nsym, sub, kw, draws, dev)
    assert calls == {"step": 50, "surv": 0}
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])
    assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and got[4] == want[4] and got[4] > 0


@pytest.mark.parametrize("S", [8, 128])
def test_batched_path_trials_take_one_launch_per_block(golden, dev, monkeypatch, S):
    """trials.eval_by_word_batched(decision='path') with 3 trials: every row equals harness.eval_by_word(fused_step=False) run alone
    on that trial; one launch of the path states step per block for all trials, mvn_vnet_decode_surv_f32 never."""
    R = 3
    tx, rx, w0, nsym, sub, kw, draws = _flow(golden, S, dev, R)
    seq = [_sequential(tx[r], rx[r], w0, S, nsym, sub, kw, draws, dev, fused_step=False) for r in range(R)]
    calls = _spy(monkeypatch)
    bank = TrialBank([w0] * R, S, SC.memory(S), dev)
    ser_b = eval_by_word_batched(bank, tx, rx, nsym, sub, [draws() for _ in range(R)], decision="path", **kw)
    assert calls == {"step": 50, "surv": 0}
    for r, (ser, wr, m, v, n) in enumerate(seq):
        assert np.array_equal(ser, ser_b[r]), (r, np.flatnonzero(ser != ser_b[r]))
        for a, b in zip(wr, bank.weights(r)):
            assert torch.equal(a, b), r
        assert torch.equal(m, bank.exp_avg[r]) and torch.equal(v, bank.exp_avg_sq[r]) and n == int(bank.step[r]), r
    assert len({tuple(row) for row in ser_b}) > 1  # the trials are not copies of each other
