"""CPU only: the by-word block steps at 256 states (mvn_vnet_byword_step_256_f32, _256_path_f32, mvn_va_byword_step_256_f32,
_256_path_f32; csrc/byword_step_256.inc) as far as they can be seen without a device -- what test_gpu_states256_step.py's word sets
put in front of the kernels (asserted on the oracle alone), the longest words and the segment lengths, the argument validation of
the four entry points in step_check's order (no case reaches a launch), the Python resolver and predicates, and the kernels'
resources from the code object."""
import ctypes

import numpy as np
import pytest

import meta_viterbinet_amd as mvn
import states256_cases as K
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

POINTERS = ("rx", "tx", "front", "dec", "msg", "enc", "lw", "labels", "nerr")
ALL = POINTERS
PAIRS = [(kind, decision) for kind in K.KINDS for decision in K.DECISIONS]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


# ------------------------------------------------------------------------------------------------------------- the word sets
def test_word_sets_reach_the_outcomes(oracle, golden):
    """Conditions on the inputs of test_gpu_states256_step.py, on the oracle alone.  Measured on the oracle: ViterbiNet (82 words)
    running 0 clean / 52 corrected / 30 failed, path 9 / 52 / 21; VA (48 words) running 0 / 19 / 29, path 5 / 17 / 26.  With G23's
    weights the running decision leaves about three bit errors per word at every SNR, so no clean word is asked of it (the
    zero-syndrome branch is byword_codec's, pinned at 16 states)."""
    ws = K.vnet_word_set(golden)
    assert ws["rx"].shape == (82, 136) and ws["msg"].shape == (82, 120)
    va = K.va_word_set()
    assert va["rx"].shape == (48, 136) and va["pri"].shape == (1, 256)
    for kind, decision in PAIRS:
        clean, corrected, failed = K.outcomes(golden, kind, decision)
        print(f"{kind} {decision}: clean {clean}, corrected {corrected}, failed {failed}")
        if kind == "vnet":
            assert corrected >= 40 and failed >= 15
        else:
            assert corrected >= 15 and failed >= 20
    differ = np.any(K.expected_set(golden, "vnet", "running")["dec"] != K.expected_set(golden, "vnet", "path")["dec"], axis=1)
    assert differ.sum() >= 40  # the path is another detection on most words
    assert np.any(K.expected_set(golden, "va", "running")["dec"] != K.expected_set(golden, "va", "path")["dec"])


def test_priors_are_compute_state_priors():
    va = mvn.VADetector(256, 8, 136, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    want = va.compute_state_priors(mvn.estimate_channel(8, 0.2, "time_decay")).cpu().numpy().T
    assert np.array_equal(K.VC.priors(256, 0.2), want)


# ------------------------------------------------------------------------------------------------------------- the longest words
def test_longest_words_and_segments(lib):
    for kind in K.KINDS:
        mx = int(getattr(lib, f"mvn_{kind}_byword_step_256_max_symbols")())
        seg = int(getattr(lib, f"mvn_{kind}_byword_step_256_segment")())
        assert 136 <= mx <= 1024 and mx % 8 == 0
        assert 16 <= seg <= mx and seg % 16 == 0
        assert mvn._lib.step256_segment(kind) == seg
    assert mvn._lib.step256_max_symbols() == int(lib.mvn_vnet_byword_step_256_max_symbols())
    assert mvn._lib.va_step256_max_symbols() == int(lib.mvn_va_byword_step_256_max_symbols())
    # the older calls keep turning 256 states down
    for name in ("mvn_vnet_byword_step_max_symbols", "mvn_vnet_byword_step_list_max_symbols", "mvn_va_byword_step_max_symbols",
                 "mvn_va_byword_step_list_max_symbols"):
        assert getattr(lib, name)(256) == 0


# ------------------------------------------------------------------------------------------------------------- validation
def call(lib, kind, decision, T=136, nsym=2, S=256, R=1, pilot=0, Bp=1, null=(), ld=None):
    """The entry point with every pointer but those in `null` non-NULL (never dereferenced: every case ends before a launch) and every
    leading dimension T but those in `ld`.  'front': the six weight arrays (with a w_stride) or state_priors."""
    p = {name: None if name in null else ctypes.c_void_p(64) for name in POINTERS}
    lds = dict({name: T for name in ("rx", "tx", "dec", "msg", "enc", "lw", "labels")}, **(ld or {}))
    front = (p["front"], Bp) if kind == "va" else (*[p["front"]] * 6, None)
    return getattr(lib, K.ENTRY[kind, decision])(
        p["rx"], lds["rx"], p["tx"], lds["tx"], *front, p["dec"], lds["dec"], p["msg"], lds["msg"], p["enc"], lds["enc"],
        p["lw"], lds["lw"], p["labels"], lds["labels"], p["nerr"], R, T, nsym, pilot, S, None)


def _table(mx):
    """(case, code for vnet, code for va) in step_check's order: shapes; the longest word; leading dimensions; rows of priors; nothing
    to do; NULL rules.  0 ok, -1 MVN_E_DIMS, -2 MVN_E_STATES, -3 MVN_E_PRIORS, -4 MVN_E_NULL."""
    D, N, OK = (-1, -1), (-4, -4), (0, 0)
    t = [
        (dict(T=135, null=ALL), D), (dict(T=135, R=0), D), (dict(T=135, Bp=0, R=0), D), (dict(T=0, nsym=1, R=0), D),
        (dict(nsym=0, null=ALL), D), (dict(nsym=9, null=ALL), D), (dict(T=16, nsym=2, null=ALL), D), (dict(T=64, nsym=8, R=0), D),
        (dict(T=72, nsym=8, R=0), OK), (dict(R=-1, null=ALL), D),
        (dict(T=mx + 8, R=0), D), (dict(T=mx + 8, null=ALL), D), (dict(T=mx, R=0), OK), (dict(T=mx, null=ALL), N),
        (dict(T=mx + 8, pilot=1, R=0), D),
        (dict(null=ALL, ld={"rx": 135}), D), (dict(R=0, ld={"rx": 135}), D), (dict(R=0, ld={"rx": 135}, null=("rx",)), D),
        (dict(R=0, ld={"tx": 119}), D), (dict(R=0, ld={"tx": 119}, null=("tx",)), D), (dict(Bp=0, R=0, ld={"enc": 135}), D),
    ]
    for name, short in (("dec", 135), ("msg", 119), ("enc", 135), ("lw", 135), ("labels", 135)):
        t += [(dict(R=0, ld={name: short}), D), (dict(R=0, ld={name: short}, null=(name,)), OK), (dict(R=0, ld={name: short + 1}), OK)]
    t += [
        (dict(Bp=0, R=0), (0, -3)), (dict(Bp=-1, R=0, pilot=1), (0, -3)), (dict(Bp=0, null=ALL), (-4, -3)),
        (dict(R=0), OK), (dict(R=0, null=ALL), OK), (dict(R=0, pilot=1, null=("rx", "front")), OK), (dict(R=0, null=("tx",)), OK),
        (dict(null=ALL), N), (dict(null=("rx",)), N), (dict(null=("tx",)), N), (dict(null=("front",)), N),
        (dict(pilot=1, null=("tx",)), N), (dict(pilot=1, null=("rx", "tx")), N), (dict(pilot=1, null=("front", "tx")), N),
        (dict(pilot=1, null=("front",), R=0), OK),
    ]
    return t


def test_entry_points_validate_in_the_documented_order(lib):
    wrong = []
    table = _table(int(lib.mvn_vnet_byword_step_256_max_symbols()))
    assert int(lib.mvn_va_byword_step_256_max_symbols()) == int(lib.mvn_vnet_byword_step_256_max_symbols())
    assert len(table) >= 50
    for case, codes in table:
        for kind, code in zip(K.KINDS, codes):
            assert code != 0 or case.get("R", 1) == 0, (case, kind)  # no case reaches a launch: the pointers are not memory
            for decision in K.DECISIONS:
                got = call(lib, kind, decision, **case)
                if got != code:
                    wrong.append((case, kind, decision, got, code))
    assert not wrong, "(case, kind, decision, returned, expected): " + "; ".join(map(repr, wrong))


@pytest.mark.parametrize("S", [2, 16, 128, 255, 512, 0, -4])
def test_other_state_counts_are_refused_first(lib, S):
    for kind, decision in PAIRS:
        for case in (dict(null=ALL), dict(R=0), dict(T=135, R=0), dict(T=135, null=ALL), dict(Bp=0, R=0), dict(R=-1)):
            assert call(lib, kind, decision, S=S, **case) == -2, (kind, decision, case)


def test_older_entry_points_still_refuse_256_states(lib):
    import test_va_states_host as VH

    for decision in ("running", "path", "list"):
        assert VH.call(lib, decision, S=256, R=0) == -2
        assert VH.call(lib, decision, S=256, R=0, entry=VH.OLD[decision]) == -2
    p = ctypes.c_void_p(64)
    for name in ("mvn_vnet_byword_step_states_f32", "mvn_vnet_byword_step_states_path_f32", "mvn_vnet_byword_step_f32",
                 "mvn_vnet_byword_step_path_f32"):
        assert getattr(lib, name)(p, 136, p, 136, p, p, p, p, p, p, None, p, 136, p, 136, p, 136, p, 136, p, 136, p, 0, 136, 2, 0, 256,
                                  None) == -2, name


# ------------------------------------------------------------------------------------------------------------- routing
class _Cuda:
    """What the predicates look at of the received words: a shape and is_cuda."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


class _Host(_Cuda):
    is_cuda = False


def _va(T, val_words=1, S=256):
    return mvn.VADetector(S, int(np.log2(S)), T, val_words, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})


def _vnet(T, S=256):
    return mvn.VNETDetector(S, {"train": T, "val": T})


def test_resolver_with_and_without_the_switch(lib):
    B = mvn._lib.BywordStep
    for kind, decision in PAIRS:
        step = B(kind, decision, 136, 2, n_states=256, states_256=True)
        assert step.name == K.ENTRY[kind, decision] and step.n_states == 256
        assert B(kind, decision, 136, 2, n_states=256, states_path=True, states_list=True, states_va=True,
                 states_256=True).name == K.ENTRY[kind, decision]
    # without the switch: as before -- the ViterbiNet names of the other state counts (which answer MVN_E_STATES), ValueError for VA
    assert B("vnet", "running", 136, 2, n_states=256).name == "mvn_vnet_byword_step_states_f32"
    assert B("vnet", "path", 136, 2, n_states=256, states_path=True).name == "mvn_vnet_byword_step_states_path_f32"
    for decision in K.DECISIONS:
        with pytest.raises(ValueError):
            B("va", decision, 136, 2, n_states=256, states_va=True)
        with pytest.raises(ValueError):
            B("va", decision, 136, 2, n_states=256)
    # the list has no step at 256 states, with the switch or without
    for kind in K.KINDS:
        with pytest.raises(ValueError):
            B(kind, "list", 136, 2, 4, n_states=256, states_path=True, states_list=True, states_va=True, states_256=True)
    # the switch changes nothing at the other state counts
    assert B("vnet", "running", 136, 2, n_states=16, states_256=True).name == "mvn_vnet_byword_step_f32"
    assert B("vnet", "path", 136, 2, n_states=64, states_path=True, states_256=True).name == "mvn_vnet_byword_step_states_path_f32"
    assert B("va", "path", 136, 2, n_states=64, states_va=True, states_256=True).name == "mvn_va_byword_step_states_path_f32"
    with pytest.raises(ValueError):
        B("va", "path", 136, 2, n_states=64, states_256=True)


def test_predicate_under_each_condition(lib, monkeypatch):
    from meta_viterbinet_amd import harness

    applies = harness._step256_applies
    monkeypatch.setattr(harness, "_STEP256_DEFAULT", {pair: True for pair in PAIRS})  # the conditions, whatever the defaults are
    T = 136
    for decision in K.DECISIONS:
        # VA: the 16-state VA rule
        assert applies(_va(T), _Cuda(1, T), 2, False, decision)
        assert applies(_va(T, 5), _Cuda(1, T), 2, True, decision)        # the word's own row
        assert not applies(_va(T, 5), _Cuda(1, T), 2, False, decision)   # several rows, no block number
        assert not applies(_va(T + 8), _Cuda(1, T), 2, False, decision)  # the detector's length is not the word's
        assert not applies(_va(T), _Host(1, T), 2, False, decision)
        assert not applies(_va(T + 4), _Cuda(1, T + 4), 2, False, decision)  # no whole bytes
        assert not applies(_va(T), _Cuda(1, T), 0, False, decision) and not applies(_va(T), _Cuda(1, T), 9, False, decision)
        assert applies(_va(72), _Cuda(1, 72), 8, False, decision) and not applies(_va(64), _Cuda(1, 64), 8, False, decision)
        mx = mvn._lib.va_step256_max_symbols()
        assert applies(_va(mx), _Cuda(1, mx), 2, False, decision) and not applies(_va(mx + 8), _Cuda(1, mx + 8), 2, False, decision)
        # ViterbiNet: the 16-state ViterbiNet rule
        assert applies(_vnet(T), _Cuda(1, T), 2, False, decision)
        assert not applies(_vnet(T), _Cuda(1, T), 2, True, decision)       # no block number for ViterbiNet
        assert not applies(_vnet(T + 8), _Cuda(1, T), 2, False, decision)  # the 'val' length is not the word's
        assert not applies(_vnet(T), _Host(1, T), 2, False, decision)
        assert not applies(_vnet(T + 4), _Cuda(1, T + 4), 2, False, decision)
        assert not applies(_vnet(T), _Cuda(1, T), 0, False, decision) and not applies(_vnet(T), _Cuda(1, T), 9, False, decision)
        assert applies(_vnet(72), _Cuda(1, 72), 8, False, decision) and not applies(_vnet(64), _Cuda(1, 64), 8, False, decision)
        mx = mvn._lib.step256_max_symbols()
        assert applies(_vnet(mx), _Cuda(1, mx), 2, False, decision) and not applies(_vnet(mx + 8), _Cuda(1, mx + 8), 2, False, decision)
        for other in (2, 16, 128):
            assert not applies(_va(T, S=other), _Cuda(1, T), 2, False, decision)
            assert not applies(_vnet(T, S=other), _Cuda(1, T), 2, False, decision)
    for det in (_va(T), _vnet(T)):
        assert not applies(det, _Cuda(1, T), 2, False, "list") and not applies(det, _Cuda(1, T), 2, False, "soft")
    assert not applies(object(), _Cuda(1, T), 2, False, "running")
    # a pair that is not a default keeps the separate launches
    monkeypatch.setattr(harness, "_STEP256_DEFAULT", {pair: pair != ("va", "path") for pair in PAIRS})
    assert not applies(_va(T), _Cuda(1, T), 2, False, "path") and applies(_va(T), _Cuda(1, T), 2, False, "running")


def test_pinned_functions_answer_as_before(lib):
    """The older predicates for a 256-state detector: what they answered before the step existed (eval_by_word consults the new
    predicate first); decision='list' at 256 states keeps raising."""
    import torch

    from meta_viterbinet_amd.harness import (_fused_step_applies, _list_step_bytes, _states_list_step_applies,
                                             _va_states_step_applies)

    T = 136
    for det in (_va(T), _vnet(T)):
        for decision in ("running", "path", "list"):
            for pass_count in (False, True):
                assert not _fused_step_applies(det, _Cuda(1, T), 2, pass_count, decision)
                assert not _va_states_step_applies(det, _Cuda(1, T), 2, pass_count, decision)
        assert not _states_list_step_applies(det, _Cuda(1, T), 2, False)
        with pytest.raises(ValueError, match="16-state"):
            _list_step_bytes(det, _Cuda(1, T), 2, False, True, None)
        with pytest.raises(ValueError):
            mvn.eval_by_word(det, torch.zeros(4, 120), torch.zeros(4, 136), 8.0, 0.2, 2, 2, decision="list")


# ------------------------------------------------------------------------------------------------------------- resources
KERNELS = {("vnet", "running"): "byword_step_256_kernel", ("vnet", "path"): "byword_path_step_256_kernel",
           ("va", "running"): "byword_step_256_va_kernel", ("va", "path"): "byword_path_step_256_va_kernel"}


def test_kernels_fit_the_cu(lib, resources):  # noqa: F811
    """The eight instantiations exist, none uses scratch, at most 256 VGPRs (two waves per SIMD), and static LDS plus the dynamic
    bytes of the longest word -- one segment of 1 KB rows and, for the path, 16 B of survivors per stage -- stays within 160 KB."""
    for (kind, decision), base in KERNELS.items():
        mx, seg = int(getattr(lib, f"mvn_{kind}_byword_step_256_max_symbols")()), mvn._lib.step256_segment(kind)
        dynamic = 4 * 256 * min(seg, mx) + (16 * mx if decision == "path" else 0)
        for NS in (2, 8):
            n = f"{base}<{NS}>"
            assert n in resources, n
            total = resources[n]["lds"] + dynamic
            print(n, resources[n], "segment", seg, "max symbols", mx, "LDS at the longest word", total)
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            assert resources[n]["vgpr"] <= 256, f"{n}: {resources[n]['vgpr']} VGPRs, two waves per SIMD leave 256"
            assert total <= 163840, f"{n}: {total} bytes of LDS at T = {mx}"
