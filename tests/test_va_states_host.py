"""CPU only: the classical Viterbi detector's by-word block steps at 4, 8, 32, 64 and 128 states (mvn_va_byword_step_states_f32,
_path_f32, _list_f32; csrc/byword_step_states_va.inc) as far as they can be seen without a device -- what
test_gpu_va_states_step.py's word sets put in front of the kernels (asserted on the oracle alone), the argument validation of the
three entry points in the documented order (no case reaches a launch), the Python resolver and predicates, and the kernels'
resources from the code object."""
import ctypes
import re

import numpy as np
import pytest

import meta_viterbinet_amd as mvn
import states_list_cases as LSC
import va_states_cases as VC
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

DECISIONS = ("running", "path", "list")
OLD = {"running": "mvn_va_byword_step_f32", "path": "mvn_va_byword_step_path_f32", "list": "mvn_va_byword_step_list_f32"}
POINTERS = ("rx", "tx", "priors", "dec", "msg", "enc", "lw", "labels", "nerr", "delta", "choice")
ALL = POINTERS


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


# ------------------------------------------------------------------------------------------------------------- the word sets
@pytest.mark.parametrize("S", VC.STATES)
def test_word_sets_reach_every_outcome(oracle, S):
    """Conditions on the inputs of test_gpu_va_states_step.py, on the oracle alone: the running decisions leave >= 5 corrected and >= 5
    failed words, the path >= 5 clean, >= 5 corrected and >= 5 failed; the list changes its mind on >= 5 words and loses no word the
    path decodes; the kernel's form of delta (alpha half-image, in-lane min of beta) is the definition's, and its sign is the path."""
    ws = VC.word_set(S)
    assert ws["rx"].shape == (48, 136) and ws["msg"].shape == (48, 120) and ws["pri"].shape == (1, S)
    run, path = VC.outcomes(S, "running"), VC.outcomes(S, "path")
    lst = VC.expected_set(S, "list")
    moved, failed = int(np.sum(lst["choice"] != 0)), int(np.sum(lst["nerr"] > 0))
    print(f"S={S}: running clean/corrected/failed {run}, path {path}, list failed {failed}, choice != 0 on {moved}")
    assert run[1] >= 5 and run[2] >= 5
    assert path[0] >= 5 and path[1] >= 5 and path[2] >= 5
    assert moved >= 5
    assert not np.any((lst["path_nerr"] == 0) & (lst["nerr"] > 0)), "the list lost a word the path decodes"
    assert failed <= path[2]
    assert np.array_equal(LSC.delta_by_halves(lst["alpha"], lst["beta"]), lst["delta"])
    assert np.array_equal((lst["delta"] < 0).astype(np.float32), lst["dec"])
    assert np.array_equal(lst["dec"], VC.expected_set(S, "path")["dec"])
    assert np.any(VC.expected_set(S, "running")["dec"] != lst["dec"])


@pytest.mark.parametrize("S", VC.STATES)
def test_priors_are_compute_state_priors(S):
    """va_states_cases.priors restates VADetector.compute_state_priors on estimate_channel's time-decay taps."""
    L = VC.SC.memory(S)
    va = mvn.VADetector(S, L, 136, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    for gamma in (0.2, 0.35):
        want = va.compute_state_priors(mvn.estimate_channel(L, gamma, "time_decay")).cpu().numpy().T
        assert np.array_equal(VC.priors(S, gamma), want)


# ------------------------------------------------------------------------------------------------------------- validation
def call(lib, decision, T=136, nsym=2, S=8, R=1, pilot=0, m=4, Bp=1, null=(), ld=None, entry=None):
    """The entry point with every pointer but those in `null` non-NULL (never dereferenced: every case ends before a launch) and every
    leading dimension T but those in `ld`."""
    p = {name: None if name in null else ctypes.c_void_p(64) for name in POINTERS}
    lds = dict({name: T for name in ("rx", "tx", "dec", "msg", "enc", "lw", "labels", "delta")}, **(ld or {}))
    tail = (m, p["delta"], lds["delta"], p["choice"]) if decision == "list" else ()
    return getattr(lib, entry or VC.ENTRY[decision])(
        p["rx"], lds["rx"], p["tx"], lds["tx"], p["priors"], Bp, p["dec"], lds["dec"], p["msg"], lds["msg"], p["enc"], lds["enc"],
        p["lw"], lds["lw"], p["labels"], lds["labels"], p["nerr"], R, T, nsym, pilot, S, *tail, None)


def _ends_before_a_launch(decision, case):
    null, pilot = case.get("null", ()), case.get("pilot", 0)
    no_tx = "tx" in null and (decision != "list" or pilot or not {"nerr", "lw", "labels"} <= set(null))
    return case.get("R", 1) == 0 or ("rx" in null and not pilot) or no_tx or ("priors" in null and not pilot)


def _table(lib, S):
    """(case, codes of (running, path, list)) in the documented order: states; shapes; the longest word; the list's limits; leading
    dimensions; rows of priors; nothing to do; NULL rules.  0 ok, -1 MVN_E_DIMS, -2 MVN_E_STATES, -3 MVN_E_PRIORS, -4 MVN_E_NULL."""
    mx, lmx = int(lib.mvn_va_byword_step_max_symbols(S)), int(lib.mvn_va_byword_step_list_max_symbols(S))
    assert lmx <= mx and lmx % 8 == 0 and mx % 8 == 0
    D, N, OK = (-1, -1, -1), (-4, -4, -4), (0, 0, 0)
    t = [
        # shapes, before everything but the state count (Bp = 0, R = 0 and NULL pointers do not get there first)
        (dict(T=135, null=ALL), D), (dict(T=135, R=0), D), (dict(T=135, Bp=0, R=0), D), (dict(T=0, nsym=1, m=1, R=0), D),
        (dict(nsym=0, m=1, null=ALL), D), (dict(nsym=9, m=9, null=ALL), D), (dict(T=16, nsym=2, m=2, null=ALL), D),
        (dict(T=64, nsym=8, m=8, R=0), D), (dict(T=72, nsym=8, m=8, R=0), OK), (dict(R=-1, null=ALL), D),
        # the longest word of the rule
        (dict(T=mx + 8, R=0), D), (dict(T=mx + 8, null=ALL), D), (dict(T=mx, R=0), (0, 0, 0 if mx == lmx else -1)),
        (dict(T=mx, null=ALL), (-4, -4, -4 if mx == lmx else -1)), (dict(T=lmx, R=0), OK), (dict(T=lmx + 8, R=0), (0, 0, -1)),
        (dict(T=lmx + 8, null=ALL), (-4, -4, -1)), (dict(T=lmx + 8, pilot=1, R=0), (0, 0, -1)),
        # the list's limits
        (dict(m=1, R=0), (0, 0, -1)), (dict(m=18, R=0), (0, 0, -1)), (dict(m=12, R=0), (0, 0, -1)), (dict(m=11, R=0), OK),
        (dict(m=12, null=ALL), (-4, -4, -1)), (dict(m=12, pilot=1, R=0), (0, 0, -1)), (dict(R=0, ld={"delta": 135}), (0, 0, -1)),
        (dict(R=0, ld={"delta": 135}, null=("delta",)), OK), (dict(m=12, Bp=0, R=0), (-3, -3, -1)),
        # leading dimensions
        (dict(null=ALL, ld={"rx": 135}), D), (dict(R=0, ld={"rx": 135}), D), (dict(R=0, ld={"rx": 135}, null=("rx",)), D),
        (dict(R=0, ld={"tx": 119}), D), (dict(R=0, ld={"tx": 119}, null=("tx",)), (-1, -1, 0)),
        (dict(R=0, pilot=1, ld={"tx": 119}, null=("tx",)), D), (dict(Bp=0, R=0, ld={"enc": 135}), D),
    ]
    for name, short in (("dec", 135), ("msg", 119), ("enc", 135), ("lw", 135), ("labels", 135)):
        t += [(dict(R=0, ld={name: short}), D), (dict(R=0, ld={name: short}, null=(name,)), OK), (dict(R=0, ld={name: short + 1}), OK)]
    t += [
        # rows of priors, before R = 0 and before any pointer
        (dict(Bp=0, R=0), (-3, -3, -3)), (dict(Bp=-1, R=0, pilot=1), (-3, -3, -3)), (dict(Bp=0, null=ALL), (-3, -3, -3)),
        # nothing to do
        (dict(R=0), OK), (dict(R=0, null=ALL), OK), (dict(R=0, pilot=1, null=("rx", "priors")), OK), (dict(R=0, null=("tx",)), OK),
        # NULL rules
        (dict(null=ALL), N), (dict(null=("rx",)), N), (dict(null=("tx",)), N), (dict(null=("priors",)), N),
        (dict(pilot=1, null=("tx",)), N), (dict(pilot=1, null=("rx", "tx")), N), (dict(pilot=1, null=("priors", "tx")), N),
        (dict(null=("tx", "rx", "nerr", "lw", "labels")), N), (dict(null=("tx", "nerr", "labels")), N), (dict(null=("tx", "nerr", "lw")), N),
        (dict(null=("tx", "priors", "nerr", "lw", "labels")), N),
    ]
    return t


@pytest.mark.parametrize("S", VC.STATES)
def test_entry_points_validate_in_the_documented_order(lib, S):
    wrong = []
    table = _table(lib, S)
    assert len(table) >= 60
    for case, codes in table:
        for decision, code in zip(DECISIONS, codes):
            assert _ends_before_a_launch(decision, case) or code in (-1, -2, -3), (case, decision)
            got = call(lib, decision, S=S, **case)
            if got != code:
                wrong.append((case, decision, got, code))
    assert not wrong, "(case, decision, returned, expected): " + "; ".join(map(repr, wrong))


@pytest.mark.parametrize("S", [2, 12, 256, 0, -4, 1024])
def test_other_state_counts_are_refused_first(lib, S):
    assert lib.mvn_va_byword_step_max_symbols(S) == 0 and lib.mvn_va_byword_step_list_max_symbols(S) == 0
    for decision in DECISIONS:
        for case in (dict(null=ALL), dict(R=0), dict(T=135, R=0), dict(T=135, null=ALL), dict(Bp=0, R=0), dict(m=12, R=0), dict(R=-1)):
            assert call(lib, decision, S=S, **case) == -2, (decision, case)


def test_longest_words(lib):
    """What the 160 KB hold next to the codec's state: no W3 image, so longer words than ViterbiNet's at 64 and 128 states."""
    run = {S: int(lib.mvn_va_byword_step_max_symbols(S)) for S in (4, 8, 16, 32, 64, 128)}
    lst = {S: int(lib.mvn_va_byword_step_list_max_symbols(S)) for S in (4, 8, 16, 32, 64, 128)}
    assert run == {4: 1024, 8: 1024, 16: 1024, 32: 1024, 64: 624, 128: 312}
    assert lst == {4: 512, 8: 512, 16: 512, 32: 512, 64: 384, 128: 192}
    for S in VC.STATES:
        assert run[S] >= mvn._lib.step_max_symbols(S) and lst[S] >= mvn._lib.list_max_symbols(S)
        assert mvn._lib.va_step_max_symbols(S) == run[S] and mvn._lib.va_list_max_symbols(S) == lst[S]


def test_sixteen_states_forward_to_the_sixteen_state_steps(lib):
    cases = [dict(null=ALL), dict(R=0), dict(T=135, null=ALL), dict(T=1024, R=0), dict(T=1032, R=0), dict(T=520, R=0), dict(nsym=9, R=0),
             dict(null=("tx",)), dict(pilot=1, null=("rx", "priors"), R=0), dict(R=0, ld={"enc": 135}), dict(null=("priors",)),
             dict(Bp=0, R=0), dict(R=-1, null=ALL), dict(m=12, R=0)]
    for decision in DECISIONS:
        for case in cases:
            assert call(lib, decision, S=16, **case) == call(lib, decision, S=16, entry=OLD[decision], **case), (decision, case)
        assert call(lib, decision, S=16, null=ALL) == -4 and call(lib, decision, S=16, R=0) == 0 and call(lib, decision, S=16, Bp=0, R=0) == -3


def test_sixteen_state_entry_points_still_refuse_other_state_counts(lib):
    for decision in DECISIONS:
        for S in VC.STATES:
            assert call(lib, decision, S=S, R=0, entry=OLD[decision]) == -2


# ------------------------------------------------------------------------------------------------------------- routing
class _Cuda:
    """What the predicates look at of the received words: a shape and is_cuda."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


class _Host(_Cuda):
    is_cuda = False


def _va(S, T, val_words=1):
    return mvn.VADetector(S, VC.SC.memory(S), T, val_words, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})


def test_resolver_finds_the_new_symbols(lib):
    B = mvn._lib.BywordStep
    for decision in DECISIONS:
        m = 4 if decision == "list" else None
        step = B("va", decision, 136, 2, m, n_states=8, states_va=True)
        assert step.name == VC.ENTRY[decision] and step.n_states == 8
        assert B("va", decision, 136, 2, m, n_states=8, states_path=True, states_list=True, states_va=True).name == VC.ENTRY[decision]
        assert B("va", decision, 136, 2, m, n_states=16, states_va=True).name == OLD[decision]
        with pytest.raises(ValueError):  # without the switch: as before
            B("va", decision, 136, 2, m, n_states=8)
        with pytest.raises(ValueError):
            B("va", decision, 136, 2, m, n_states=8, states_path=True, states_list=True)
        with pytest.raises(ValueError):  # 2 and 256 states: not served, with the switch or without
            B("va", decision, 136, 2, m, n_states=256, states_va=True)
    # the switch changes nothing for ViterbiNet
    assert B("vnet", "path", 136, 2, n_states=8, states_path=True, states_va=True).name == "mvn_vnet_byword_step_states_path_f32"
    with pytest.raises(ValueError):
        B("vnet", "path", 136, 2, n_states=8, states_va=True)


@pytest.mark.parametrize("S", VC.STATES)
def test_predicate_under_each_condition(lib, S):
    from meta_viterbinet_amd.harness import _va_states_step_applies as applies

    T = 136
    for decision in DECISIONS:
        assert applies(_va(S, T), _Cuda(1, T), 2, False, decision)
        assert applies(_va(S, T, 5), _Cuda(1, T), 2, True, decision)        # the word's own row
        assert not applies(_va(S, T, 5), _Cuda(1, T), 2, False, decision)   # several rows, no block number
        assert not applies(_va(S, T + 8), _Cuda(1, T), 2, False, decision)  # the detector's length is not the word's
        assert not applies(_va(S, T), _Host(1, T), 2, False, decision)
        assert not applies(_va(S, T + 4), _Cuda(1, T + 4), 2, False, decision)  # no whole bytes
        assert not applies(_va(S, T), _Cuda(1, T), 0, False, decision) and not applies(_va(S, T), _Cuda(1, T), 9, False, decision)
        assert applies(_va(S, 72), _Cuda(1, 72), 8, False, decision) and not applies(_va(S, 64), _Cuda(1, 64), 8, False, decision)
        mx = mvn._lib.va_list_max_symbols(S) if decision == "list" else mvn._lib.va_step_max_symbols(S)
        assert applies(_va(S, mx), _Cuda(1, mx), 2, False, decision)
        assert not applies(_va(S, mx + 8), _Cuda(1, mx + 8), 2, False, decision)
    assert not applies(_va(S, T), _Cuda(1, T), 2, False, "soft")
    for other in (2, 16, 256):
        assert not applies(_va(other, T), _Cuda(1, T), 2, False, "path")
    vnet = mvn.VNETDetector(S, {"train": T, "val": T})
    assert not applies(vnet, _Cuda(1, T), 2, False, "running")


@pytest.mark.parametrize("S", VC.STATES)
def test_pinned_functions_answer_as_before(lib, S):
    """_fused_step_applies, _states_list_step_applies and _list_step_bytes for a VADetector off 16 states: what they answered before
    the step existed (eval_by_word consults the new predicate first)."""
    from meta_viterbinet_amd.harness import _fused_step_applies, _list_step_bytes, _states_list_step_applies

    T = 136
    va = _va(S, T)
    for decision in DECISIONS:
        assert not _fused_step_applies(va, _Cuda(1, T), 2, False, decision) and not _fused_step_applies(va, _Cuda(1, T), 2, True, decision)
    assert not _states_list_step_applies(va, _Cuda(1, T), 2, False)
    with pytest.raises(ValueError, match="16-state"):
        _list_step_bytes(va, _Cuda(1, T), 2, False, True, None)


def test_list_refusals_name_the_condition(lib):
    """decision='list' has no other route: eval_by_word says which condition of the step does not hold."""
    import torch

    from meta_viterbinet_amd.harness import _va_states_list_conditions as conditions

    with pytest.raises(ValueError, match="192"):
        conditions(_va(128, 200), _Cuda(1, 200), 2, False, True)
    with pytest.raises(ValueError, match="transmission_length"):
        conditions(_va(8, 144), _Cuda(1, 136), 2, False, True)
    with pytest.raises(ValueError, match="pass_count"):
        conditions(_va(8, 136, 5), _Cuda(1, 136), 2, False, True)
    conditions(_va(8, 136), _Cuda(1, 136), 2, False, True)
    with pytest.raises(ValueError, match="fused_step"):
        mvn.eval_by_word(_va(8, 136), torch.zeros(4, 120), torch.zeros(4, 136), 8.0, 0.2, 2, 2, decision="list", fused_step=False)
    with pytest.raises(ValueError, match="192"):
        mvn.list_decode(_va(128, 200), torch.zeros(2, 200), 2, gamma=0.2)
    with pytest.raises(ValueError, match="gamma"):
        mvn.list_decode(_va(8, 136), torch.zeros(2, 136), 2)


# ------------------------------------------------------------------------------------------------------------- resources
KERNELS = {"running": "byword_step_states_va_kernel", "path": "byword_path_step_states_va_kernel",
           "list": "byword_list_step_states_va_kernel"}


def test_kernels_fit_the_cu(lib, resources):  # noqa: F811
    """All thirty instantiations exist, none uses scratch, and static LDS plus the dynamic bytes of the longest word stays within a
    CU's 160 KB."""
    for decision, base in KERNELS.items():
        names = sorted(n for n in resources if re.fullmatch(base + r"<\d+, \d+>", n))
        assert names == sorted(f"{base}<{S}, {NS}>" for S in VC.STATES for NS in (2, 8))
        for S in VC.STATES:
            if decision == "list":
                max_T = int(lib.mvn_va_byword_step_list_max_symbols(S))
                per_symbol = 4 * S + 2 * S + (4 if S <= 32 else 8)
            else:
                max_T = int(lib.mvn_va_byword_step_max_symbols(S))
                per_symbol = 4 * S
            assert max_T >= 136 and max_T % 8 == 0
            for NS in (2, 8):
                n = f"{base}<{S}, {NS}>"
                total = resources[n]["lds"] + per_symbol * max_T
                print(n, resources[n], "max symbols", max_T, "LDS at the longest word", total)
                assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
                assert total <= 163840, f"{n}: {total} bytes of LDS at T = {max_T}"
                assert resources[n]["vgpr"] <= 256, f"{n}: {resources[n]['vgpr']} VGPRs, two waves per SIMD leave 256"
