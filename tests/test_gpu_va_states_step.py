"""GPU tests (pytest -m gpu) of the classical Viterbi detector's by-word block steps at 4, 8, 32, 64 and 128 states
(mvn_va_byword_step_states_f32, _path_f32, _list_f32; csrc/byword_step_states_va.inc) through the raw ctypes symbols, and of the
public routes that take them (harness.eval_by_word with a VADetector at these state counts, ecc.list_decode).  Every comparison is
exact (np.array_equal; delta included: -0 equals +0).  The expected values come from va_states_cases -- the C oracle's costs, running
decisions, survivors, traceback and codec, and the list referee of states_list_cases on those costs; tests/test_va_states_host.py
shows on the CPU what the word sets put in front of the kernels."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import va_states_cases as VC
from step_call import SENTINEL, step
from test_gpu_states_step import REQUESTS

pytestmark = pytest.mark.gpu

DECISIONS = ("running", "path", "list")
FLAT = ("nerr", "choice")
SC = VC.SC


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    assert mvn._lib.load().mvn_device_info(None, None, None, 0) == 0
    return torch.device("cuda:0")


def _names(decision):
    return VC.LIST_OUTPUTS if decision == "list" else VC.OUTPUTS


def _check(tag, out, row, exp, names):
    """The requested outputs' rows equal the expected step's, and every padding element kept its sentinel."""
    for name in names:
        if name not in out or exp.get(name) is None:
            continue
        got = out[name] if name in FLAT else out[name][:, :row[name]]
        if not np.array_equal(got, exp[name]):
            idx = np.argwhere(got != exp[name])
            pytest.fail(f"{tag}: {name}{idx[0].tolist()} = {got[tuple(idx[0])]}, expected {exp[name][tuple(idx[0])]}; "
                        f"{len(idx)} elements differ")
        if name not in FLAT:
            assert np.all(out[name][:, row[name]:] == SENTINEL[name]), f"{tag}: padding of {name} written"


def _va(S, T, dev, val_words=1):
    return mvn.VADetector(S, SC.memory(S), T, val_words, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})


# ------------------------------------------------------------------------------------------------------------- the word sets
@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("S", VC.STATES)
def test_word_set_in_one_launch(oracle, dev, S, decision):
    """All 48 words in one launch with one row of priors: dec, msg, nerr, enc, label word and labels (list: delta and choice too) are
    the referee's.  Then three words alone (R = 1).  The running dec is also mvn_va_decode_f32's, the path's VADetector.viterbi_path's."""
    ws = VC.word_set(S)
    exp = VC.expected_set(S, decision)
    out, row = VC.launch(dev, decision, S, ws["rx"], ws["msg"], ws["nsym"], ws["pri"])
    _check(f"S={S} {decision} R=48", out, row, exp, _names(decision))
    for r in (0, int(np.flatnonzero(exp["nerr"] > 0)[0]), int(np.flatnonzero(exp["nerr"] == 0)[-1])):
        one, _ = VC.launch(dev, decision, S, ws["rx"][r:r + 1], ws["msg"][r:r + 1], ws["nsym"], ws["pri"])
        for name in _names(decision):
            assert np.array_equal(one[name], out[name][r:r + 1]), (S, decision, r, name)
    va = _va(S, VC.T_WORD, dev)
    y = torch.as_tensor(ws["rx"]).to(dev)
    assert torch.equal(va._priors_table(y, VC.GAMMA, "val", None).cpu(), torch.as_tensor(ws["pri"]))
    if decision == "running":
        assert np.array_equal(va(y, "val", 8.0, VC.GAMMA).cpu().numpy(), exp["dec"]), "mvn_va_decode_f32 against the oracle"
    else:
        assert np.array_equal(va.viterbi_path(y, 8.0, VC.GAMMA).cpu().numpy(), exp["dec"]), "viterbi_path against the oracle"


# ------------------------------------------------------------------------------------------------------------- priors indexing
@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("R,gammas", [(6, (0.05, 0.1, 0.2, 0.3, 0.5, 0.8)), (6, (0.1, 0.2, 0.6)), (1, (0.35,))], ids=["Bp6", "Bp3", "R1"])
@pytest.mark.parametrize("S", VC.STATES)
def test_word_r_uses_row_r_mod_bp(oracle, dev, S, R, gammas, decision):
    """Every word on its own channel (Bp = R), two words per channel (row r % Bp), one word."""
    case = VC.small_case(S, 136, 2, R=R, gammas=gammas)
    assert case["pri"].shape == (len(gammas), S) and len({p.tobytes() for p in case["pri"]}) == len(gammas)
    exp = VC.expected(case, decision)
    out, row = VC.launch(dev, decision, S, case["rx"], case["msg"], 2, case["pri"])
    _check(f"S={S} {decision} Bp={len(gammas)}", out, row, exp, _names(decision))
    if len(gammas) == 6:  # the rows matter: with row 0 for every word some decision differs
        wrong = VC.expected(dict(case, pri=case["pri"][:1]), decision)
        assert any(not np.array_equal(wrong[n], exp[n], equal_nan=True) for n in ("dec", "delta") if n in exp)


# ------------------------------------------------------------------------------------------------------------- edge shapes
def _longest(S, decision):
    return mvn._lib.va_list_max_symbols(S) if decision == "list" else mvn._lib.va_step_max_symbols(S)


@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("shape", ["shortest", "nsym8", "word", "longest"])
@pytest.mark.parametrize("S", VC.STATES)
def test_edge_shapes(oracle, dev, S, shape, decision):
    """T = 16 with nsym = 1 (one tile, the shortest word); T = 72 with nsym = 8 (the NS = 8 instantiation); T = 136; the rule's longest
    word (the last byte of the image)."""
    T, nsym = {"shortest": (16, 1), "nsym8": (72, 8), "word": (136, 2), "longest": (_longest(S, decision), 2)}[shape]
    m = min(nsym + 2, T // 8) if nsym < 8 else 9
    case = VC.small_case(S, T, nsym, R=3)
    exp = VC.expected(case, decision, m)
    out, row = VC.launch(dev, decision, S, case["rx"], case["msg"], nsym, case["pri"], m=m)
    _check(f"S={S} {decision} T={T} nsym={nsym}", out, row, exp, _names(decision))


@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("S", VC.STATES)
def test_every_leading_dimension(oracle, dev, S, decision):
    """Every *_ld larger than its row and all of them different; NaN in rx's padding and 7 in tx's."""
    ws = VC.word_set(S)
    T, K = VC.T_WORD, VC.T_WORD - 16
    ld = {"rx": T + 3, "tx": K + 5, "dec": T + 1, "msg": K + 2, "enc": T + 7, "lw": T + 4, "labels": T + 6, "delta": T + 9}
    sel = slice(20, 28)
    out, row = VC.launch(dev, decision, S, ws["rx"][sel], ws["msg"][sel], 2, ws["pri"], ld=ld)
    exp = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[0] == VC.WORDS else v) for k, v in VC.expected_set(S, decision).items()}
    _check(f"S={S} {decision} ld", out, row, exp, _names(decision))


NULL_IN_TURN = [tuple(n for n in VC.LIST_OUTPUTS if n != out) for out in VC.LIST_OUTPUTS]


@pytest.mark.parametrize("want", REQUESTS + NULL_IN_TURN, ids=lambda w: "+".join(w))
@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("S", [8, 128])
def test_some_outputs_only(oracle, dev, S, decision, want):
    """Outputs not requested are NULL: test_gpu_states_step.py's sets, and each output NULL in turn."""
    want = tuple(n for n in want if n in _names(decision))
    ws = VC.word_set(S)
    sel = slice(0, 12)
    out, row = VC.launch(dev, decision, S, ws["rx"][sel], ws["msg"][sel], 2, ws["pri"], want=want)
    assert sorted(out) == sorted(want)
    exp = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[0] == VC.WORDS else v) for k, v in VC.expected_set(S, decision).items()}
    _check(f"S={S} {decision} want={want}", out, row, exp, want)


def test_list_step_without_a_transmitted_word(oracle, dev):
    """tx NULL on the list's data step when nothing is compared with it: a decoder without a genie."""
    for S in (4, 64):
        ws = VC.word_set(S)
        exp = VC.expected_set(S, "list")
        out, row = VC.launch(dev, "list", S, ws["rx"], None, 2, ws["pri"], want=("dec", "msg", "enc", "delta", "choice"))
        _check(f"S={S} no tx", out, row, exp, ("dec", "msg", "delta", "choice"))
        chosen = exp["candidates"][np.arange(VC.WORDS), exp["choice"]]
        assert np.array_equal(out["enc"], chosen)


@pytest.mark.parametrize("entry", DECISIONS)
@pytest.mark.parametrize("nsym", [2, 8])
@pytest.mark.parametrize("S", VC.STATES)
def test_pilot_step(oracle, dev, S, nsym, entry):
    """A pilot through each of the three entry points, rx and state_priors NULL: enc = label word = rs_encode(tx), nerr 0, labels at the
    word's own memory length; dec, msg, delta and choice untouched."""
    tx = VC.word_set(S)["msg"][:5, :VC.T_WORD - 8 * nsym]
    out, row = VC.launch(dev, entry, S, None, tx, nsym, None, pilot=True, m=min(nsym + 2, 9))
    exp = VC.expected_pilot(tx, nsym, S)
    _check(f"S={S} pilot via {entry}", out, row, exp, ("nerr", "enc", "lw", "labels"))
    assert not out["nerr"].any()
    for name in ("dec", "msg") + (("delta", "choice") if entry == "list" else ()):
        assert np.all(out[name] == SENTINEL[name]), name


# ------------------------------------------------------------------------------------------------------------- torch.min's rule
def _odd_case(S, odd):
    """Eight words of the set with one thing non-finite, or an exact tie at every stage."""
    ws = VC.word_set(S)
    rx, msg, pri = ws["rx"][:8].copy(), ws["msg"][:8], ws["pri"].copy()
    T = rx.shape[1]
    if odd == "nan_prior":
        pri[0, S // 2 + 1] = np.nan
    elif odd == "inf_priors":
        pri[0, 1], pri[0, S - 2] = np.inf, -np.inf
    elif odd == "nan_first_sample":
        rx[:, 0] = np.nan
    elif odd == "nan_middle_sample":
        rx[:, T // 2] = np.nan
    elif odd == "nan_last_sample":
        rx[:, T - 1] = np.nan
    elif odd == "inf_samples":
        rx[:, 3], rx[:, T // 2 + 1], rx[0::2, T - 2] = np.inf, -np.inf, np.inf
    else:
        # ties: a channel whose only tap is the current symbol's (priors -1 and +1 by the state's lowest bit: every value exact), the
        # noise-free word, and every third sample 0 -- halfway between the two priors.  A stage's costs then take two values, or one:
        # path metrics tie all over the trellis, in the ACS, in the running argmin and in the final argmin
        pri = VC.priors(S, h=[0.0] * (SC.memory(S) - 1) + [1.0])
        rx = (1.0 - 2.0 * ws["cw"][:8]).astype(np.float32)
        rx[:, ::3] = 0.0
    return dict(rx=rx, msg=msg, pri=pri, nsym=2, S=S)


ODD = ["nan_prior", "inf_priors", "nan_first_sample", "nan_middle_sample", "nan_last_sample", "inf_samples", "ties"]


@pytest.mark.parametrize("decision", DECISIONS)
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("S", VC.STATES)
def test_odd_costs_follow_torch_min(oracle, dev, S, odd, decision):
    """A NaN prior (a partial-NaN cost at every stage), infinite priors, NaN and infinite samples, and exact ties between candidates
    (the first index wins): running and path steps are the oracle's (torch.min: NaN when either candidate is; torch.argmin: the first
    NaN is minimal) in every output; the list step holds dec to the path's rule and stays in range."""
    case = _odd_case(S, odd)
    cost = VC.costs(case)
    if odd == "ties":
        cand = VC.LSC.soft(cost)[0][:, :-1] + cost  # the ACS candidates: those of predecessors 2 k and 2 k + 1 are neighbours
        tied = cand[:, :, 0::2] == cand[:, :, 1::2]
        assert set(np.unique(case["pri"])) == {-1.0, 1.0} and tied[:, ::3].all() and not tied[:, 1::3].any()
    elif odd == "nan_prior":
        bad = np.isnan(cost)
        assert bad.any(axis=2).all() and not bad.all(axis=2).any()
    else:
        assert not np.isfinite(cost).all()
    if decision == "list" and odd != "ties":
        exp = VC.expected(case, "path")
        out, row = VC.launch(dev, "list", S, case["rx"], case["msg"], 2, case["pri"])
        _check(f"S={S} list {odd}", out, row, exp, ("dec",))
        assert np.all((out["choice"] >= 0) & (out["choice"] <= 6)) and np.all((out["labels"] >= 0) & (out["labels"] < S))
        assert np.all((out["nerr"] >= 0) & (out["nerr"] <= 120))
        for name in ("msg", "enc", "lw"):
            assert np.all((out[name][:, :row[name]] == 0) | (out[name][:, :row[name]] == 1)), name
        return
    exp = VC.expected(case, decision)
    out, row = VC.launch(dev, decision, S, case["rx"], case["msg"], 2, case["pri"])
    _check(f"S={S} {decision} {odd}", out, row, exp, _names(decision))


# ------------------------------------------------------------------------------------------------------------- 16 states
@pytest.mark.parametrize("decision", DECISIONS)
def test_sixteen_states_equal_the_sixteen_state_steps(oracle, dev, decision):
    case = VC.small_case(16, 136, 2, R=6, gammas=(0.1, 0.2, 0.6))
    pri = torch.as_tensor(case["pri"]).to(dev)
    for pilot in (False, True):
        new, _ = VC.launch(dev, decision, 16, case["rx"], case["msg"], 2, case["pri"], pilot=pilot)
        old, _ = step(dev, decision, "va", case["rx"], case["msg"], 2, pilot, m=4, pri=pri, Bp=3)
        for name in _names(decision):
            assert np.array_equal(new[name], old[name]), (pilot, name)


# ------------------------------------------------------------------------------------------------------------- public interface
def _eval(det, ws, dev, **kw):
    return mvn.eval_by_word(det, torch.as_tensor(ws["msg"]).to(dev), torch.as_tensor(ws["rx"]).to(dev), 8.0, VC.GAMMA, 2, VC.WORDS + 1, **kw)


@pytest.mark.parametrize("decision", ["running", "path"])
@pytest.mark.parametrize("S", VC.STATES)
def test_eval_by_word_takes_the_step_and_changes_no_result(oracle, dev, monkeypatch, S, decision):
    """eval_by_word(VADetector at S) without updates: the default route launches the new step once per data block and returns what
    fused_step=False (the separate launches) returns and what the referee counts, exactly."""
    ws = VC.word_set(S)
    exp = VC.expected_set(S, decision)
    det = _va(S, VC.T_WORD, dev)
    lib = mvn._lib.load()
    calls = {"step": 0}
    fn = getattr(lib, VC.ENTRY[decision])

    def counted(*a):
        calls["step"] += 1
        return fn(*a)

    monkeypatch.setattr(lib, VC.ENTRY[decision], counted)
    ser = _eval(det, ws, dev, decision=decision)
    assert calls["step"] == VC.WORDS - 1  # block 0 is a pilot
    separate = _eval(det, ws, dev, decision=decision, fused_step=False)
    assert calls["step"] == VC.WORDS - 1
    assert np.array_equal(ser, separate)
    want = mvn.metrics.ser_from_errors(exp["nerr"], ws["msg"].shape[1])
    want[0] = 0.0
    assert np.array_equal(ser, want) and (ser > 0).sum() >= 5


@pytest.mark.parametrize("S", VC.STATES)
def test_eval_by_word_list(oracle, dev, S):
    """decision='list' with a VADetector off 16 states: the referee's error counts over K in the reference's arithmetic; with the
    block number passed (a table of several rows, every word on its own) the same."""
    ws = VC.word_set(S)
    exp = VC.expected_set(S, "list")
    want = mvn.metrics.ser_from_errors(exp["nerr"], ws["msg"].shape[1])
    want[0] = 0.0
    ser = _eval(_va(S, VC.T_WORD, dev), ws, dev, decision="list")
    assert np.array_equal(ser, want)
    assert (ser > 0).sum() < (_eval(_va(S, VC.T_WORD, dev), ws, dev, decision="path") > 0).sum()  # the list's gain against the baseline
    ser = _eval(_va(S, VC.T_WORD, dev, val_words=VC.WORDS), ws, dev, decision="list", pass_count=True)
    assert np.array_equal(ser, want)


@pytest.mark.parametrize("S", VC.STATES)
def test_list_decode(oracle, dev, S):
    ws = VC.word_set(S)
    exp = VC.expected_set(S, "list")
    det = _va(S, VC.T_WORD, dev)
    y = torch.as_tensor(ws["rx"]).to(dev)
    msg, choice, delta = mvn.list_decode(det, y, 2, gamma=VC.GAMMA, return_delta=True)
    assert np.array_equal(msg.cpu().numpy(), exp["msg"]) and np.array_equal(delta.cpu().numpy(), exp["delta"])
    assert np.array_equal(choice.cpu().numpy(), exp["choice"])
    two = mvn.list_decode(det, y, 2, list_bytes=4, gamma=VC.GAMMA)
    assert len(two) == 2 and torch.equal(two[0], msg) and torch.equal(two[1], choice)  # the default m is n_symbols + 2
    with pytest.raises(ValueError, match="divide"):  # B divisible by the rows of priors
        mvn.list_decode(_va(S, VC.T_WORD, dev, val_words=5), y, 2, gamma=VC.GAMMA)
