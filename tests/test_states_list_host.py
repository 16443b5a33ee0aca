"""CPU only: the by-word LIST step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_list_f32,
byword_list_step_states_kernel<S, NS>) as far as it can be seen without a device -- what test_gpu_states_list.py's word sets put in
front of the kernel (asserted on the referee alone, states_list_cases.py), the two identities the kernel's LDS plan rests on, the
argument validation of the entry point (no case reaches a launch: R = 0 or a required pointer NULL), the longest word per state count,
the Python predicate, resolver and call sites with the refusals that remain, and the kernels' resources from the code object."""
import ctypes
import re

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
import states_list_cases as LS
import states_step_cases as SC
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)
from test_step_validation_host import ALL, WEIGHTS
from test_step_validation_host import call as call16

ENTRY = LS.ENTRY
POINTERS = tuple(n for n in ALL if n != "priors")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


# ------------------------------------------------------------------------------------------------------------- the word sets
# S: (words, failed on the path, failed on the list, path-decoded words lost, words with choice != 0), m = 4
RECORDED = {4: (64, 12, 6, 0, 12), 8: (50, 2, 0, 0, 2), 32: (50, 9, 1, 0, 9), 64: (50, 6, 2, 0, 6), 128: (50, 15, 5, 0, 15)}


@pytest.mark.parametrize("S", SC.STATES)
def test_word_sets_show_the_list_decoder_at_work(oracle, golden, S):
    """Conditions on the inputs of test_gpu_states_list.py, on the referee alone: the list rule fails fewer words than the path and
    loses none the path decodes, at least 2 words are not the hard decoder's, no two different codewords tie in metric, no delta is 0
    and its sign is the traced-back word -- and the two identities of the kernel's LDS plan hold bit for bit."""
    ref = LS.expected_set(golden, S)
    path_failed, list_failed = ref["path_nerr"] > 0, ref["nerr"] > 0
    got = (ref["dec"].shape[0], int(path_failed.sum()), int(list_failed.sum()), int((list_failed & ~path_failed).sum()),
           int((ref["choice"] != 0).sum()))
    print(f"S={S}: words, failed on the path, failed on the list, lost, choice != 0 = {got}")
    assert got == RECORDED[S]
    assert got[3] == 0 and got[4] >= 2 and got[2] < got[1]
    M, cands = ref["metrics"], ref["candidates"]
    for r in range(M.shape[0]):
        order = np.argsort(M[r], kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            assert M[r, a] != M[r, b] or np.array_equal(cands[r, a], cands[r, b]), (S, r, a, b)
    delta = ref["delta"]
    assert np.all(np.isfinite(delta)) and not np.any(delta == 0)
    assert np.array_equal((delta < 0).astype(np.float32), ref["dec"])
    H = S // 2
    assert np.array_equal(ref["alpha"][..., :H], ref["alpha"][..., H:])
    assert np.array_equal(LS.delta_by_halves(ref["alpha"], ref["beta"]), delta)
    assert ref["labels"].max() == S - 1 and ref["labels"].min() == 0


def test_referee_at_sixteen_states_is_list_cases(oracle):
    """soft() and metrics() with S = 16 are list_cases.py's."""
    import list_cases as LC

    rng = np.random.RandomState(16)
    cost = rng.standard_normal((3, 24, 16)).astype(np.float32)
    for a, b in zip(LS.soft(cost), LC.soft(cost)):
        assert np.array_equal(a, b)
    words = rng.randint(0, 2, (3, 5, 24)).astype(np.float32)
    assert np.array_equal(LS.metrics(cost, words), LC.metrics(cost, words))


# ------------------------------------------------------------------------------------------------------------- validation
def call(lib, T=136, nsym=2, S=8, R=1, pilot=0, m=4, null=(), ld=None, name=ENTRY):
    """The entry point with every pointer but those in `null` non-NULL (never dereferenced: the case ends before a launch; w_stride,
    which the host would read, is always NULL) and every leading dimension T but those in `ld`."""
    p = {n: None if n in null else ctypes.c_void_p(64) for n in POINTERS}
    lds = dict({n: T for n in ("rx", "tx", "dec", "msg", "enc", "lw", "labels", "delta")}, **(ld or {}))
    return getattr(lib, name)(p["rx"], lds["rx"], p["tx"], lds["tx"], *[p[w] for w in WEIGHTS], None, p["dec"], lds["dec"], p["msg"],
                              lds["msg"], p["enc"], lds["enc"], p["lw"], lds["lw"], p["labels"], lds["labels"], p["nerr"], R, T, nsym,
                              pilot, S, m, p["delta"], lds["delta"], p["choice"], None)


def _table(mx):
    """(case, code) at one served state count, in the documented order of the checks: 0 ok, -1 MVN_E_DIMS, -4 MVN_E_NULL."""
    t = [
        # shapes and the list's limits, before any leading dimension or pointer
        (dict(T=135, null=ALL), -1), (dict(T=135, R=0), -1), (dict(nsym=0, m=1, null=ALL), -1), (dict(nsym=9, m=9, null=ALL), -1),
        (dict(T=16, nsym=2, null=ALL), -1), (dict(T=64, nsym=8, m=8, R=0), -1), (dict(T=72, nsym=8, m=8, R=0), 0),
        (dict(T=mx + 8, null=ALL), -1), (dict(T=mx + 8, R=0), -1), (dict(T=mx, R=0), 0), (dict(T=mx, null=ALL), -4),
        (dict(R=-1, null=ALL), -1), (dict(m=1, null=ALL), -1), (dict(m=18, null=ALL), -1), (dict(m=12, null=ALL), -1),
        (dict(m=11, null=ALL), -4), (dict(m=11, R=0), 0), (dict(m=12, R=0), -1), (dict(nsym=1, m=17, R=0), 0),
        (dict(T=128, nsym=8, m=10, R=0), 0), (dict(T=128, nsym=8, m=11, R=0), -1),
        (dict(R=0, ld={"delta": 135}), -1), (dict(R=0, ld={"delta": 135}, null=("delta",)), 0),
        # a pilot is checked against the list's limits first
        (dict(R=0, pilot=1, m=12), -1), (dict(R=0, pilot=1, ld={"delta": 135}), -1), (dict(R=0, pilot=1, T=mx + 8), -1),
        # leading dimensions
        (dict(null=ALL, ld={"rx": 135}), -1), (dict(R=0, ld={"rx": 135}), -1), (dict(R=0, ld={"tx": 119}), -1),
        (dict(R=0, ld={"tx": 119}, null=("tx",)), 0), (dict(R=0, pilot=1, ld={"tx": 119}, null=("tx",)), -1),
        # nothing to do
        (dict(R=0), 0), (dict(R=0, null=ALL), 0), (dict(R=0, pilot=1, null=("rx",)), 0),
        # pointers
        (dict(null=ALL), -4), (dict(null=("rx",)), -4), (dict(null=("tx",)), -4), (dict(null=("tx", "nerr", "labels")), -4),
        (dict(null=("tx", "nerr", "lw")), -4), (dict(null=("tx", "rx", "nerr", "lw", "labels")), -4),
        (dict(pilot=1, null=("tx",)), -4), (dict(pilot=1, null=("tx", "nerr", "lw", "labels")), -4),
    ]
    for name, short in (("dec", 135), ("msg", 119), ("enc", 135), ("lw", 135), ("labels", 135)):
        t += [(dict(R=0, ld={name: short}), -1), (dict(R=0, ld={name: short}, null=(name,)), 0)]
    for w in WEIGHTS:
        t += [(dict(null=(w,)), -4), (dict(pilot=1, null=(w,)), -4)]
    return t


def test_list_states_entry_argument_validation(lib):
    wrong = []
    for S in (2, 12, 256, 0, -4):  # the state count comes first
        for case in (dict(null=ALL), dict(R=0), dict(T=135, R=0), dict(T=135, null=ALL), dict(m=99, R=0)):
            if call(lib, S=S, **case) != -2:
                wrong.append((S, case, call(lib, S=S, **case), -2))
    for S in SC.STATES:
        mx = int(lib.mvn_vnet_byword_step_list_max_symbols(S))
        table = _table(mx)
        assert len(table) >= 60
        for case, code in table:
            null = case.get("null", ())
            assert case.get("R", 1) <= 0 or "rx" in null or "tx" in null or any(w in null for w in WEIGHTS), case  # no launch
            got = call(lib, S=S, **case)
            if got != code:
                wrong.append((S, case, got, code))
    assert not wrong, "(S, case, returned, expected): " + "; ".join(map(repr, wrong))


def test_sixteen_states_forward_to_the_sixteen_state_list_step(lib):
    cases = [dict(null=ALL), dict(R=0), dict(T=135, null=ALL), dict(T=512, R=0), dict(T=520, R=0), dict(nsym=9, m=9, R=0),
             dict(m=12, R=0), dict(m=11, R=0), dict(null=("tx",)), dict(pilot=1, null=("rx",), R=0), dict(R=0, ld={"enc": 135}),
             dict(R=0, ld={"delta": 135}), dict(null=("W3",)), dict(R=-1, null=ALL), dict(R=0, ld={"tx": 119}, null=("tx",))]
    for case in cases:
        assert call(lib, S=16, **case) == call16(lib, "vnet", "list", S=16, **case), case
    assert call(lib, S=16, null=ALL) == -4 and call(lib, S=16, R=0) == 0 and call(lib, S=16, T=520, R=0) == -1


def test_sixteen_state_list_entry_keeps_refusing_other_state_counts(lib):
    for S in SC.STATES:
        assert call16(lib, "vnet", "list", S=S, R=0) == -2


def test_list_max_symbols(lib):
    """What the LDS holds next to the static part at 6 S + 4 (8 above 32 states) bytes per symbol, at most 512 (the ranking takes a
    byte per lane): at least the reference's word of 136 at every state count, a multiple of 8, no more than the path step's bound,
    512 at 16 states (the step it forwards to), 0 where the step does not exist."""
    got = {S: int(lib.mvn_vnet_byword_step_list_max_symbols(S)) for S in (1, 2, 4, 8, 12, 16, 32, 64, 128, 256, 0, -4)}
    print(got)
    for S in SC.STATES:
        assert 136 <= got[S] <= 512 and got[S] % 8 == 0 and got[S] <= int(lib.mvn_vnet_byword_step_max_symbols(S))
        assert mvn._lib.list_max_symbols(S) == got[S]
    assert got[4] == got[8] == got[32] == 512 and got[64] >= got[128]
    assert got[16] == 512
    assert all(got[S] == 0 for S in (1, 2, 12, 256, 0, -4))


# ------------------------------------------------------------------------------------------------------------- routing
class _Cuda:
    """What the predicates look at of the received words: a shape and is_cuda."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


def _vnet(S, T):
    return mvn.VNETDetector(S, {"train": T, "val": T})


@pytest.mark.parametrize("S", SC.STATES)
def test_predicate_takes_the_list_at_every_state_count(lib, S):
    from meta_viterbinet_amd.harness import _fused_step_applies, _list_step_bytes, _states_list_step_applies
    from meta_viterbinet_amd.trials import _lock_step_serves

    T, long = SC.T_WORD, mvn._lib.list_max_symbols(S) + 8
    assert _states_list_step_applies(_vnet(S, T), _Cuda(1, T), 2, False)
    assert _list_step_bytes(_vnet(S, T), _Cuda(1, T), 2, False, True, None) == 4
    assert _list_step_bytes(_vnet(S, T), _Cuda(1, T), 2, False, True, 6) == 6
    assert not _states_list_step_applies(_vnet(S, long), _Cuda(1, long), 2, False)
    assert not _states_list_step_applies(_vnet(S, T), _Cuda(1, T), 2, True)        # a block number
    assert not _states_list_step_applies(_vnet(S, T + 8), _Cuda(1, T), 2, False)   # 'val' length != word length
    assert not _states_list_step_applies(_vnet(S, T), _Cuda(1, T), 9, False)
    assert not _states_list_step_applies(_vnet(16, T), _Cuda(1, T), 2, False)      # 16 states: _fused_step_applies' own
    # the predicates pinned before this step existed stay as they were
    assert not _fused_step_applies(_vnet(S, T), _Cuda(1, T), 2, False, "list")
    assert not _lock_step_serves(S, _Cuda(3, 50, T), 2, "list", False)
    with pytest.raises(ValueError, match=str(mvn._lib.list_max_symbols(S)) if long <= 512 else "512"):
        _list_step_bytes(_vnet(S, long), _Cuda(1, long), 2, False, True, None)
    with pytest.raises(ValueError, match="fused_step"):
        _list_step_bytes(_vnet(S, T), _Cuda(1, T), 2, False, False, None)
    with pytest.raises(ValueError, match="block number"):
        _list_step_bytes(_vnet(S, T), _Cuda(1, T), 2, True, True, None)
    va = mvn.VADetector(S, SC.memory(S), T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    assert not _states_list_step_applies(va, _Cuda(1, T), 2, False)
    with pytest.raises(ValueError, match="16-state"):
        _list_step_bytes(va, _Cuda(1, T), 2, False, True, None)


@pytest.mark.parametrize("S", [2, 256])
def test_two_and_256_states_have_no_list_step(lib, S):
    from meta_viterbinet_amd.harness import _list_step_bytes, _states_list_step_applies

    T = SC.T_WORD
    assert not _states_list_step_applies(_vnet(S, T), _Cuda(1, T), 2, False)
    with pytest.raises(ValueError, match="16-state"):
        _list_step_bytes(_vnet(S, T), _Cuda(1, T), 2, False, True, None)
    with pytest.raises(ValueError, match="list_decode"):
        mvn.list_decode(_vnet(S, T), torch.zeros(2, T), 2)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", T, 2, 4, n_states=S, states_path=True, states_list=True)


def test_evaluations_refuse_what_the_list_step_does_not_serve(lib):
    det = _vnet(8, 136)
    tx, rx = torch.zeros(2, 120), torch.zeros(2, 136)
    with pytest.raises(ValueError, match="ROCm"):  # words on the CPU: no other route to fall back to
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="list")
    with pytest.raises(ValueError, match="fused_step"):
        mvn.eval_by_word(det, tx, rx, 8.0, 0.2, 2, 4, decision="list", fused_step=False)
    with pytest.raises(ValueError, match="512"):
        mvn.eval_by_word(_vnet(8, 520), torch.zeros(2, 504), torch.zeros(2, 520), 8.0, 0.2, 2, 4, decision="list")
    long = mvn._lib.list_max_symbols(128) + 8
    with pytest.raises(ValueError, match=str(long - 8)):
        mvn.list_decode(_vnet(128, long), torch.zeros(2, long), 2)

    class _Bank:  # (what eval_by_word_batched looks at before it refuses)
        def __init__(self, S):
            self.n_states, self.R = S, 1

    for S, T, what in ((256, 136, "states"), (2, 136, "states"), (128, long, str(long - 8)), (8, 136, "ROCm")):
        with pytest.raises(ValueError, match=what):
            mvn.eval_by_word_batched(_Bank(S), torch.zeros(1, 2, T - 16), torch.zeros(1, 2, T), 2, 4, [None], decision="list")


def test_resolver_finds_the_list_symbol(lib):
    step = mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=8, states_path=True, states_list=True)
    assert step.name == ENTRY and step.n_states == 8 and step.list_bytes == 4
    assert ctypes.cast(step.fn, ctypes.c_void_p).value == ctypes.cast(getattr(lib, ENTRY), ctypes.c_void_p).value
    both = dict(states_path=True, states_list=True)
    assert mvn._lib.BywordStep("vnet", "running", 136, 2, n_states=8, **both).name == LS.RUNNING_ENTRY
    assert mvn._lib.BywordStep("vnet", "path", 136, 2, n_states=8, **both).name == LS.PATH_ENTRY
    assert mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=16, **both).name == "mvn_vnet_byword_step_list_f32"
    assert mvn._lib.BywordStep("va", "list", 136, 2, 4, n_states=16, **both).name == "mvn_va_byword_step_list_f32"
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("va", "list", 136, 2, 4, n_states=8, **both)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", 136, 2, None, n_states=8, **both)  # list_bytes belongs to it
    # the pinned refusals of the calls without the switch
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=8)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=8, states_path=True)


def test_call_sites_resolve_through_the_one_resolver(lib):
    import inspect

    from meta_viterbinet_amd import trials
    from meta_viterbinet_amd.harness import _block_step

    for S in SC.STATES:
        assert _block_step(_vnet(S, 136), 136, 2, "list", 4).name == ENTRY
    assert _block_step(_vnet(16, 136), 136, 2, "list", 4).name == "mvn_vnet_byword_step_list_f32"
    assert _block_step(_vnet(64, 136), 136, 2, "path", None).name == LS.PATH_ENTRY
    assert "states_list=True" in inspect.getsource(trials._cohort_steps)


# ------------------------------------------------------------------------------------------------------------- resources
def test_list_step_kernels_fit_the_cu(lib, resources):  # noqa: F811
    """The ten instantiations exist, use no scratch and at most 256 VGPRs (two waves per SIMD), and their static LDS plus the dynamic
    part of the longest word -- logits 4 S, alpha half-image 2 S, survivors 4 (8 above 32 states) bytes per symbol -- stays within a
    CU's 160 KB."""
    names = sorted(n for n in resources if re.fullmatch(r"byword_list_step_states_kernel<\d+, \d+>", n))
    assert names == sorted(f"byword_list_step_states_kernel<{S}, {NS}>" for S in SC.STATES for NS in (2, 8))
    for S in SC.STATES:
        max_T = int(lib.mvn_vnet_byword_step_list_max_symbols(S))
        for NS in (2, 8):
            n = f"byword_list_step_states_kernel<{S}, {NS}>"
            total = resources[n]["lds"] + (6 * S + (4 if S <= 32 else 8)) * max_T
            print(n, resources[n], "max symbols", max_T, "LDS at the longest word", total)
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            assert resources[n]["vgpr"] <= 256, f"{n}: {resources[n]['vgpr']} VGPRs, two waves per SIMD leave 256"
            assert total <= 163840, f"{n}: {total} bytes of LDS at T = {max_T}"
