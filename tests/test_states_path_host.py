"""CPU only: the by-word PATH step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_path_f32,
byword_path_step_states_kernel<S, NS>) as far as it can be seen without a device -- the argument validation of the entry point
against the running entry point's (no case reaches a launch), what test_gpu_states_path.py's word sets put in front of the kernel
(asserted on the oracle alone), the Python predicates and the resolver, and the kernels' resources from the code object."""
import ctypes
import re

import numpy as np
import pytest

import meta_viterbinet_amd as mvn
import states_path_cases as PC
import states_step_cases as SC
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)
from test_states_step_host import ALL, WEIGHTS, call

RUNNING, PATH = PC.RUNNING_ENTRY, PC.ENTRY


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


# ------------------------------------------------------------------------------------------------------------- validation
def _validation_cases(lib):
    """test_states_step_host.py::test_states_step_argument_validation's table, as keyword sets of call()."""
    cases = []
    for S in (2, 12, 256):
        cases += [dict(S=S, null=ALL), dict(S=S, R=0), dict(S=S, T=135, R=0), dict(S=S, T=135, null=ALL)]
    for S in SC.STATES:
        mx = int(lib.mvn_vnet_byword_step_max_symbols(S))
        cases += [dict(S=S, T=135, null=ALL), dict(S=S, T=135, R=0), dict(S=S, nsym=0, null=ALL), dict(S=S, nsym=9, null=ALL),
                  dict(S=S, T=16, nsym=2, null=ALL), dict(S=S, T=64, nsym=8, R=0), dict(S=S, T=72, nsym=8, R=0),
                  dict(S=S, T=mx + 8, null=ALL), dict(S=S, T=mx + 8, R=0), dict(S=S, R=-1, null=ALL), dict(S=S, null=ALL, ld={"rx": 135}),
                  dict(S=S, R=0, ld={"rx": 135}), dict(S=S, R=0, ld={"tx": 119})]
        for name, short in (("dec", 135), ("msg", 119), ("enc", 135), ("lw", 135), ("labels", 135)):
            cases += [dict(S=S, R=0, ld={name: short}), dict(S=S, R=0, ld={name: short}, null=(name,))]
        cases += [dict(S=S, R=0), dict(S=S, R=0, null=ALL), dict(S=S, T=mx, R=0), dict(S=S, T=mx, null=ALL), dict(S=S, null=ALL),
                  dict(S=S, null=("rx",)), dict(S=S, null=("tx",)), dict(S=S, pilot=1, null=("tx",))]
        for w in WEIGHTS:
            cases += [dict(S=S, null=(w,)), dict(S=S, pilot=1, null=(w,))]
    return cases


def test_path_entry_validates_like_the_running_entry(lib):
    """The same code as mvn_vnet_byword_step_states_f32 for every case of its validation table (same checks, same order); the literal
    codes for one case each."""
    wrong = []
    cases = _validation_cases(lib)
    assert len(cases) > 200
    for case in cases:
        got, want = call(lib, PATH, **case), call(lib, RUNNING, **case)
        if got != want:
            wrong.append((case, got, want))
    assert not wrong, "(case, path entry, running entry): " + "; ".join(map(repr, wrong))
    assert call(lib, PATH, S=12, R=0) == -2
    assert call(lib, PATH, S=8, T=135, R=0) == -1
    assert call(lib, PATH, S=8, R=0) == 0
    assert call(lib, PATH, S=8, null=("rx",)) == -4
    for S in SC.STATES:  # one bound for both steps
        mx = int(lib.mvn_vnet_byword_step_max_symbols(S))
        assert call(lib, PATH, S=S, T=mx, R=0) == 0 and call(lib, PATH, S=S, T=mx + 8, R=0) == -1


def test_sixteen_states_forward_to_the_sixteen_state_path_step(lib):
    cases = [dict(null=ALL), dict(R=0), dict(T=135, null=ALL), dict(T=1024, R=0), dict(T=1032, R=0), dict(nsym=9, R=0),
             dict(null=("tx",)), dict(pilot=1, null=("rx",), R=0), dict(R=0, ld={"enc": 135}), dict(null=("W3",)), dict(R=-1, null=ALL)]
    for case in cases:
        assert call(lib, PATH, S=16, **case) == call(lib, "mvn_vnet_byword_step_path_f32", S=16, **case), case
    assert call(lib, PATH, S=16, null=ALL) == -4 and call(lib, PATH, S=16, R=0) == 0 and call(lib, PATH, S=16, T=1032, R=0) == -1


# ------------------------------------------------------------------------------------------------------------- the word sets
RECORDED = {4: (32, 20, 12), 8: (39, 9, 2), 32: (17, 24, 9), 64: (16, 28, 6), 128: (4, 31, 15)}


@pytest.mark.parametrize("S", SC.STATES)
def test_word_sets_reach_every_outcome_under_the_path(oracle, golden, S):
    """Per state count, on the oracle alone: >= 2 words the decoder fails on, >= 4 without a byte error, >= 8 it corrects, and the path
    differs from the running decisions on >= 40 words -- conditions on the inputs of test_gpu_states_path.py."""
    ws = PC.word_set(golden, S)
    path, running, ref = PC.detected(golden, S)
    clean, corrected, failed = PC.outcomes(golden, S)
    differ = int(np.any(path != running, axis=1).sum())
    print(f"S={S}: {path.shape[0]} words, clean {clean}, corrected {corrected}, failed {failed}; path != running on {differ}")
    assert path.shape == (64 if S == 4 else 50, SC.T_WORD)
    assert failed >= 2 and clean >= 4 and corrected >= 8 and differ >= 40
    assert (clean, corrected, failed) == RECORDED[S]
    assert np.array_equal(ref["label_word"][ref["nerr"] > 0], path[ref["nerr"] > 0])
    assert np.array_equal(ref["label_word"][ref["nerr"] == 0], ws["cw"][ref["nerr"] == 0])


def test_four_state_set_keeps_the_running_sets_messages_and_weights(oracle, golden):
    a, b = PC.word_set(golden, 4), SC.word_set(golden, 4)
    assert np.array_equal(a["msg"], b["msg"]) and np.array_equal(a["cw"], b["cw"]) and all(x is y for x, y in zip(a["w"], b["w"]))
    assert not np.array_equal(a["rx"], b["rx"])


# ------------------------------------------------------------------------------------------------------------- routing
class _Cuda:
    """What the predicates look at of the received words: a shape and is_cuda."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


@pytest.mark.parametrize("S", SC.STATES)
def test_predicates_take_the_path_at_every_state_count(lib, S):
    from meta_viterbinet_amd.harness import _fused_step_applies
    from meta_viterbinet_amd.trials import _lock_step_serves

    def vnet(T):
        return mvn.VNETDetector(S, {"train": T, "val": T})

    T, long = SC.T_WORD, mvn._lib.step_max_symbols(S) + 8
    for decision in ("running", "path"):
        assert _fused_step_applies(vnet(T), _Cuda(1, T), 2, False, decision)
        assert _lock_step_serves(S, _Cuda(3, 50, T), 2, decision, False)
        assert not _fused_step_applies(vnet(long), _Cuda(1, long), 2, False, decision)
        assert not _lock_step_serves(S, _Cuda(3, 50, long), 2, decision, False)
        assert not _fused_step_applies(vnet(T), _Cuda(1, T), 2, True, decision)      # a block number
        assert not _fused_step_applies(vnet(T + 8), _Cuda(1, T), 2, False, decision)  # 'val' length != word length
        assert not _fused_step_applies(vnet(T), _Cuda(1, T), 9, False, decision)
        assert not _fused_step_applies(vnet(T), _Cuda(1, T + 4), 2, False, decision)  # no whole bytes
    assert not _fused_step_applies(vnet(T), _Cuda(1, T), 2, False, "list")
    assert not _lock_step_serves(S, _Cuda(3, 50, T), 2, "list", False)
    assert _lock_step_serves(S, _Cuda(3, 50, T), 2, "path", True) == (S <= 32)  # the meta-learning kernel's limit stays
    L = SC.memory(S)
    va = mvn.VADetector(S, L, T, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    assert not _fused_step_applies(va, _Cuda(1, T), 2, False, "path") and not _fused_step_applies(va, _Cuda(1, T), 2, True, "path")


def test_resolver_finds_the_path_symbol(lib):
    step = mvn._lib.BywordStep("vnet", "path", 136, 2, n_states=8, states_path=True)
    assert step.name == PATH and step.n_states == 8
    assert ctypes.cast(step.fn, ctypes.c_void_p).value == ctypes.cast(getattr(lib, PATH), ctypes.c_void_p).value
    assert mvn._lib.BywordStep("vnet", "running", 136, 2, n_states=8, states_path=True).name == RUNNING
    assert mvn._lib.BywordStep("vnet", "path", 136, 2, n_states=16, states_path=True).name == "mvn_vnet_byword_step_path_f32"
    for kind, decision, m in (("va", "running", None), ("va", "path", None), ("vnet", "list", 4)):
        with pytest.raises(ValueError):
            mvn._lib.BywordStep(kind, decision, 136, 2, m, n_states=8, states_path=True)
    # the pinned refusals of the plain call
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("va", "running", 136, 2, n_states=8)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "path", 136, 2, n_states=8)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=8)


def test_call_sites_resolve_through_the_one_resolver(lib):
    from meta_viterbinet_amd.harness import _block_step

    det = mvn.VNETDetector(64, {"train": 136, "val": 136})
    assert _block_step(det, 136, 2, "path", None).name == PATH
    assert _block_step(det, 136, 2, "running", None).name == RUNNING


# ------------------------------------------------------------------------------------------------------------- resources
def test_path_step_kernels_fit_the_cu(lib, resources):  # noqa: F811
    """The ten instantiations exist, use no scratch and at most 256 VGPRs (two waves per SIMD), and their static LDS plus the image
    of the longest word -- 4 S bytes per symbol, the survivors live inside it -- stays within a CU's 160 KB.  No more static LDS than
    the running step's kernel: the one bound serves both."""
    names = sorted(n for n in resources if re.fullmatch(r"byword_path_step_states_kernel<\d+, \d+>", n))
    assert names == sorted(f"byword_path_step_states_kernel<{S}, {NS}>" for S in SC.STATES for NS in (2, 8))
    for S in SC.STATES:
        max_T = int(lib.mvn_vnet_byword_step_max_symbols(S))
        for NS in (2, 8):
            n = f"byword_path_step_states_kernel<{S}, {NS}>"
            total = resources[n]["lds"] + 4 * S * max_T
            print(n, resources[n], "max symbols", max_T, "LDS at the longest word", total)
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            assert resources[n]["vgpr"] <= 256, f"{n}: {resources[n]['vgpr']} VGPRs, two waves per SIMD leave 256"
            assert total <= 163840, f"{n}: {total} bytes of LDS at T = {max_T}"
            assert resources[n]["lds"] <= resources[f"byword_step_states_kernel<{S}, {NS}>"]["lds"]
