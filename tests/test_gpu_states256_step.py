"""GPU tests (pytest -m gpu) of the by-word block steps at 256 states (mvn_vnet_byword_step_256_f32, _256_path_f32,
mvn_va_byword_step_256_f32, _256_path_f32; csrc/byword_step_256.inc) through the raw ctypes symbols, and of harness.eval_by_word, which
takes them.  Every comparison is exact.  The expected values come from states256_cases -- the C oracle's logits, costs, running
decisions, survivors, traceback and codec; tests/test_states256_host.py shows on the CPU what the word sets put in front of the
kernels.  The shapes are taken from the kernels' own segment length (the word passes through the LDS in segments)."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import states256_cases as K
from meta_viterbinet_amd.trials import TrialBank
from step_call import SENTINEL
from test_gpu_reference_flow import RecordedDraws
from test_gpu_states_step import NULL_IN_TURN, REQUESTS

pytestmark = pytest.mark.gpu

PAIRS = [(kind, decision) for kind in K.KINDS for decision in K.DECISIONS]
pairs = pytest.mark.parametrize("kind,decision", PAIRS, ids=["-".join(p) for p in PAIRS])
S = K.S


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


def _check(tag, out, row, exp, names=K.OUTPUTS):
    """The requested outputs' rows equal the expected step's, and every padding element kept its sentinel."""
    for name in names:
        if name not in out or exp.get(name) is None:
            continue
        got = out[name] if name == "nerr" else out[name][:, :row[name]]
        if not np.array_equal(got, exp[name]):
            idx = np.argwhere(got != exp[name])
            pytest.fail(f"{tag}: {name}{idx[0].tolist()} = {got[tuple(idx[0])]}, expected {exp[name][tuple(idx[0])]}; "
                        f"{len(idx)} elements differ")
        if name != "nerr":
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{tag}: padding of {name} written"


def _front(kind, case, dev):
    return case["pri"] if kind == "va" else [torch.as_tensor(a).to(dev).contiguous() for a in case["w"]]


def _word_set(golden, kind):
    return K.vnet_word_set(golden) if kind == "vnet" else K.va_word_set()


def _rows(exp, sel):
    return {k: v[sel] for k, v in exp.items()}


def _vnet(w, T, dev):
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w):
            p.copy_(torch.as_tensor(a).reshape(p.shape))
    return det


def _va(T, dev):
    return mvn.VADetector(S, K.MEMORY, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})


# ------------------------------------------------------------------------------------------------------------- the word sets
@pairs
def test_word_set_in_one_launch(oracle, golden, dev, kind, decision):
    """The whole word set in one launch with one weight set / one row of priors: every output is the referee's.  Then three words alone
    (R = 1), bit-equal to their rows of the batch.  dec is also the library's own detection (forward('val') / viterbi_path)."""
    ws = _word_set(golden, kind)
    exp = K.expected_set(golden, kind, decision)
    front = _front(kind, ws, dev)
    out, row = K.launch(dev, kind, decision, ws["rx"], ws["msg"], ws["nsym"], front)
    _check(f"{kind} {decision} R={ws['rx'].shape[0]}", out, row, exp)
    for r in (0, int(np.flatnonzero(exp["nerr"] > 0)[0]), int(np.flatnonzero(exp["nerr"] == 0)[-1])):
        one, _ = K.launch(dev, kind, decision, ws["rx"][r:r + 1], ws["msg"][r:r + 1], ws["nsym"], front)
        for name in K.OUTPUTS:
            assert np.array_equal(one[name], out[name][r:r + 1]), (kind, decision, r, name)
    y = torch.as_tensor(ws["rx"]).to(dev)
    if kind == "vnet":
        det = _vnet(ws["w"], K.T_WORD, dev)
        with torch.no_grad():
            lib_dec = det(y, "val") if decision == "running" else det.viterbi_path(y)
    else:
        det = _va(K.T_WORD, dev)
        lib_dec = det(y, "val", 8.0, K.VC.GAMMA) if decision == "running" else det.viterbi_path(y, 8.0, K.VC.GAMMA)
    assert np.array_equal(lib_dec.cpu().numpy(), exp["dec"]), "the library's separate detection against the oracle"


@pytest.mark.parametrize("decision", K.DECISIONS)
def test_word_set_with_a_weight_set_per_word(oracle, golden, dev, decision):
    """R weight sets through w_stride (a TrialBank's rows; the sets of rows >= 1 scaled by their own factor): word r is detected with
    set r, and its codec outputs follow from ITS detection."""
    ws = K.vnet_word_set(golden)
    R = 24
    rx, msg = ws["rx"][:R], ws["msg"][:R]
    w = [[(a * np.float32(f)).astype(np.float32) for a in ws["w"]] for f in np.concatenate([[1.0], np.linspace(0.9, 1.1, R - 1)])]
    bank = TrialBank(w, S, K.MEMORY, dev)
    dec = np.concatenate([K.vnet_detect(rx[r:r + 1], w[r], decision) for r in range(R)])
    assert not np.array_equal(dec, K.expected_set(golden, "vnet", decision)["dec"][:R])  # the perturbed sets do decide differently
    ref = K.SC.expected_step(dec, msg, ws["nsym"], False, S)
    exp = dict(dec=dec, msg=ref["msg"], nerr=ref["nerr"], enc=ref["enc"], lw=ref["label_word"], labels=ref["labels"])
    wp = [ctypes.c_void_p(bank.theta.data_ptr() + 4 * int(bank.off[a])) for a in range(6)]
    out, row = K.launch(dev, "vnet", decision, rx, msg, ws["nsym"], wp, w_stride=[bank.P] * 6)
    _check(f"vnet {decision} per-word weights", out, row, exp)


@pytest.mark.parametrize("decision", K.DECISIONS)
def test_word_r_uses_row_r_mod_bp(oracle, dev, decision):
    """Bp = 2: two channels, word r on the channel of row r % 2."""
    case = K.va_small_case(136, 2, R=6, gammas=(0.1, 0.6))
    assert case["pri"].shape == (2, S) and not np.array_equal(case["pri"][0], case["pri"][1])
    exp = K.expected("va", case, decision)
    out, row = K.launch(dev, "va", decision, case["rx"], case["msg"], 2, case["pri"])
    _check(f"va {decision} Bp=2", out, row, exp)
    wrong = K.expected("va", dict(case, pri=case["pri"][:1]), decision)
    assert not np.array_equal(wrong["dec"], exp["dec"])  # the rows matter


# ------------------------------------------------------------------------------------------------------------- the smallest shapes
def _shapes(kind):
    """(T, nsym): one tile in one segment; a half-empty tile; exactly one full segment; a second segment of half a tile; the
    reference's word; the NS = 8 instantiation; three segments (metrics, survivors and the walk cross two edges); the longest word."""
    seg = mvn._lib.step256_segment(kind)
    mx = mvn._lib.step256_max_symbols() if kind == "vnet" else mvn._lib.va_step256_max_symbols()
    return [(16, 1), (24, 2), (seg, 2), (seg + 8, 2), (136, 2), (136, 8), (2 * seg + 8, 2), (mx, 2)]


SHAPE_IDS = ["one_tile", "half_tile", "one_segment", "segment_and_half_tile", "word", "nsym8", "three_segments", "longest"]


@pytest.mark.parametrize("weights", ["random", "trained"])
@pytest.mark.parametrize("shape", range(8), ids=SHAPE_IDS)
@pairs
def test_smallest_shapes(oracle, golden, dev, kind, decision, shape, weights):
    """Each shape with random and with G23's weights (ViterbiNet); for the classical detector with one and with two rows of priors."""
    T, nsym = _shapes(kind)[shape]
    if kind == "vnet":
        case = K.vnet_small_case(golden, T, nsym, weights)
    else:
        case = K.va_small_case(T, nsym, gammas=(K.VC.GAMMA,) if weights == "trained" else (0.1, 0.6))
    exp = K.expected(kind, case, decision)
    out, row = K.launch(dev, kind, decision, case["rx"], case["msg"], nsym, _front(kind, case, dev))
    _check(f"{kind} {decision} T={T} nsym={nsym} {weights}", out, row, exp)


def test_shapes_cross_the_segments():
    """What the shapes above rely on: the reference's word is longer than a ViterbiNet segment, and the longest word has many."""
    for kind in K.KINDS:
        seg = mvn._lib.step256_segment(kind)
        (_, _), (_, _), (t1, _), (t2, _), _, _, (t3, _), (mx, _) = _shapes(kind)
        assert t1 == seg and seg < t2 < 2 * seg < t3 < 3 * seg and t3 <= mx and mx >= 4 * seg
    assert mvn._lib.step256_segment("vnet") < 136


# ------------------------------------------------------------------------------------- pilot, leading dimensions, optional outputs
@pytest.mark.parametrize("nsym", [2, 8])
@pairs
def test_pilot_step(oracle, golden, dev, kind, decision, nsym):
    """A pilot through each of the four entry points, rx NULL (VA: state_priors NULL too): enc = label word = rs_encode(tx), nerr 0,
    labels at memory 8; dec and msg untouched."""
    ws = _word_set(golden, kind)
    tx = ws["msg"][:5, :K.T_WORD - 8 * nsym]
    front = None if kind == "va" else _front(kind, ws, dev)
    out, row = K.launch(dev, kind, decision, None, tx, nsym, front, pilot=True)
    _check(f"{kind} pilot via {decision}", out, row, K.expected_pilot(tx, nsym), ("nerr", "enc", "lw", "labels"))
    assert not out["nerr"].any()
    for name in ("dec", "msg"):
        assert np.all(out[name] == SENTINEL[name]), name


@pytest.mark.parametrize("pilot", [False, True])
@pairs
def test_every_leading_dimension(oracle, golden, dev, kind, decision, pilot):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's."""
    ws = _word_set(golden, kind)
    T, Kb = K.T_WORD, K.T_WORD - 16
    ld = {"rx": T + 3, "tx": Kb + 5, "dec": T + 1, "msg": Kb + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6}
    sel = slice(20, 28)
    out, row = K.launch(dev, kind, decision, ws["rx"][sel], ws["msg"][sel], 2, _front(kind, ws, dev), pilot=pilot, ld=ld)
    if pilot:
        assert np.all(out["dec"] == SENTINEL["dec"]) and np.all(out["msg"] == SENTINEL["msg"])
        _check(f"{kind} {decision} pilot ld", out, row, K.expected_pilot(ws["msg"][sel], 2), ("nerr", "enc", "lw", "labels"))
    else:
        _check(f"{kind} {decision} ld", out, row, _rows(K.expected_set(golden, kind, decision), sel))


@pytest.mark.parametrize("want", REQUESTS + NULL_IN_TURN, ids=lambda w: "+".join(w))
@pairs
def test_some_outputs_only(oracle, golden, dev, kind, decision, want):
    """Outputs not requested are NULL: the five sets of test_gpu_byword_codec.py, and each output NULL in turn."""
    ws = _word_set(golden, kind)
    sel = slice(0, 12)
    out, row = K.launch(dev, kind, decision, ws["rx"][sel], ws["msg"][sel], 2, _front(kind, ws, dev), want=want)
    assert sorted(out) == sorted(want)
    _check(f"{kind} {decision} want={want}", out, row, _rows(K.expected_set(golden, kind, decision), sel), want)


# ------------------------------------------------------------------------------------------------------------- torch.min's rule
def _long_words(kind, golden):
    """Four words longer than a segment with nsym = 2: the odd metrics cross a segment edge."""
    T = mvn._lib.step256_segment(kind) + 56
    assert T > mvn._lib.step256_segment(kind) and T % 8 == 0
    return K.vnet_small_case(golden, T, 2, "trained", R=4) if kind == "vnet" else K.va_small_case(T, 2, R=4)


@pytest.mark.parametrize("odd", ["nan_in_b3", "inf_in_W3"])
@pytest.mark.parametrize("decision", K.DECISIONS)
def test_partly_odd_logits_follow_torch_min(oracle, golden, dev, decision, odd):
    """A NaN in one entry of b3 / +inf in one row of W3: some but not all of a symbol's costs are NaN or infinite.  The decisions are
    the oracle's (torch.argmin: the first NaN is minimal; torch.min: NaN when either candidate is NaN)."""
    case = _long_words("vnet", golden)
    w = [a.copy() for a in case["w"]]
    if odd == "nan_in_b3":
        w[5][S // 2 + 1] = np.nan
    else:
        w[4][S // 2 - 1, :] = np.inf
    case = dict(case, w=w)
    logits = oracle.vnet_logits(case["rx"], w)
    bad = ~np.isfinite(logits)
    assert bad.any(axis=2).all() and not bad.all(axis=2).any()  # every symbol: some costs odd, never all
    exp = K.expected("vnet", case, decision)
    out, row = K.launch(dev, "vnet", decision, case["rx"], case["msg"], 2, _front("vnet", case, dev))
    _check(f"vnet {decision} {odd}", out, row, exp)


@pytest.mark.parametrize("odd", ["nan_prior", "inf_priors", "nan_middle_sample", "inf_samples"])
@pytest.mark.parametrize("decision", K.DECISIONS)
def test_odd_costs_follow_torch_min(oracle, dev, decision, odd):
    """A NaN prior (a partial-NaN cost at every stage), infinite priors, a NaN sample in the first segment (every later metric NaN) and
    infinite samples: every output is the oracle's."""
    case = _long_words("va", None)
    rx, pri = case["rx"].copy(), case["pri"].copy()
    T = rx.shape[1]
    if odd == "nan_prior":
        pri[0, S // 2 + 1] = np.nan
    elif odd == "inf_priors":
        pri[0, 1], pri[0, S - 2] = np.inf, -np.inf
    elif odd == "nan_middle_sample":
        rx[:, T // 2] = np.nan
    else:
        rx[:, 3], rx[:, T // 2 + 1], rx[0::2, T - 2] = np.inf, -np.inf, np.inf
    case = dict(case, rx=rx, pri=pri)
    assert not np.isfinite(K.VC.costs(case)).all()
    exp = K.expected("va", case, decision)
    out, row = K.launch(dev, "va", decision, case["rx"], case["msg"], 2, case["pri"])
    _check(f"va {decision} {odd}", out, row, exp)


# ------------------------------------------------------------------------------------------------------------- public interface
def _counted(monkeypatch, kind, decision):
    lib = mvn._lib.load()
    calls = {"step": 0}
    fn = getattr(lib, K.ENTRY[kind, decision])

    def counted(*a):
        calls["step"] += 1
        return fn(*a)

    monkeypatch.setattr(lib, K.ENTRY[kind, decision], counted)
    return calls


def _default(kind, decision):
    from meta_viterbinet_amd import harness

    return harness._STEP256_DEFAULT[kind, decision]


@pytest.mark.parametrize("decision", K.DECISIONS)
def test_eval_by_word_on_the_reference_flow(golden, dev, monkeypatch, decision):
    """G23's by-word flow with self-supervised training at 256 states: the default route and fused_step=False give the same
    ser_by_word and bit-identical final weights; with the running decision that ser is the reference's own."""
    g = golden(K.GOLDEN)
    tag = K.TAG
    ss_it, _, _, _, snr, subframes, nsym = [int(v) for v in g[f"{tag}_meta"]]
    ser_thresh = float(g[f"{tag}_ser_thresh"])
    tx = torch.tensor(g[f"{tag}_tx"], device=dev).float()
    rx = torch.tensor(g[f"{tag}_rx"], device=dev)
    T = rx.shape[1]
    w0 = [g[f"{tag}_w0_{i}"] for i in range(6)]
    calls = _counted(monkeypatch, "vnet", decision)
    got = {}
    for fused in (True, False):
        det = _vnet(w0, T, dev)
        tr = mvn.OnlineTrainer(det, 8, use_kernel=True)
        draws = RecordedDraws(g[f"{tag}_multinomial"], g[f"{tag}_randint_high"], g[f"{tag}_randint"], dev)
        before = calls["step"]
        ser = mvn.eval_by_word(det, tx, rx, float(snr), 0.2, nsym, subframes, online_trainer=tr, draws=draws, hip_meta=True,
                               graphed_meta=False, self_supervised=True, self_supervised_iterations=ss_it, ser_thresh=ser_thresh,
                               decision=decision, fused_step=fused)
        # one launch of the step per block where it is the default route, none through the separate launches
        assert calls["step"] - before == (rx.shape[0] if fused and _default("vnet", decision) else 0)
        got[fused] = (ser, [p.detach().cpu().numpy().copy() for p in det.parameters()], tr.step)
    assert np.array_equal(got[True][0], got[False][0])
    assert got[True][2] == got[False][2] > 0
    for a, b in zip(got[True][1], got[False][1]):
        assert np.array_equal(a, b)
    assert any(not np.array_equal(a, np.asarray(b, np.float32).reshape(a.shape)) for a, b in zip(got[True][1], w0))  # it trained
    if decision == "running":
        assert np.array_equal(got[True][0], g[f"{tag}_ser_by_word"])


@pytest.mark.parametrize("decision", K.DECISIONS)
def test_eval_by_word_with_a_va_detector(oracle, dev, monkeypatch, decision):
    """eval_by_word(VADetector at memory 8) over the VA word set: the default route returns what fused_step=False (the separate
    launches) returns and what the referee counts, exactly."""
    ws = K.va_word_set()
    exp = K.expected_set(None, "va", decision)
    det = _va(K.T_WORD, dev)
    calls = _counted(monkeypatch, "va", decision)
    words = ws["rx"].shape[0]
    run = lambda **kw: mvn.eval_by_word(det, torch.as_tensor(ws["msg"]).to(dev), torch.as_tensor(ws["rx"]).to(dev), 8.0, K.VC.GAMMA, 2,  # noqa: E731
                                        words + 1, decision=decision, **kw)
    ser = run()
    assert calls["step"] == (words - 1 if _default("va", decision) else 0)  # block 0 is a pilot
    separate = run(fused_step=False)
    assert calls["step"] == (words - 1 if _default("va", decision) else 0)
    assert np.array_equal(ser, separate)
    want = mvn.metrics.ser_from_errors(exp["nerr"], ws["msg"].shape[1])
    want[0] = 0.0
    assert np.array_equal(ser, want) and (ser > 0).sum() >= 5


@pytest.mark.parametrize("kind", K.KINDS)
def test_list_has_no_step_at_256_states(dev, kind):
    det = _va(K.T_WORD, dev) if kind == "va" else mvn.VNETDetector(S, {"train": K.T_WORD, "val": K.T_WORD}).to(dev)
    with pytest.raises(ValueError):
        mvn.eval_by_word(det, torch.zeros(4, 120, device=dev), torch.zeros(4, 136, device=dev), 8.0, 0.2, 2, 2, decision="list")
