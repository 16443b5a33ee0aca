"""CPU only: the by-word block step at 4, 8, 32, 64 and 128 states (mvn_vnet_byword_step_states_f32) as far as it can be seen without
a device -- what test_gpu_states_step.py's word sets put in front of the kernel (asserted on the oracle alone, so the GPU test cannot
pass vacuously), the argument validation of the new entry point (no case reaches a launch: R = 0 or a required pointer NULL), the
longest word per state count, and the Python call site."""
import ctypes

import numpy as np
import pytest

import meta_viterbinet_amd as mvn
import states_step_cases as SC

WEIGHTS = ("W1", "b1", "W2", "b2", "W3", "b3")
POINTERS = ("rx", "tx", "dec", "msg", "enc", "lw", "labels", "nerr") + WEIGHTS
ALL = POINTERS


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


# ------------------------------------------------------------------------------------------------------------- the word sets
@pytest.mark.parametrize("S", SC.STATES)
def test_word_sets_reach_every_outcome(oracle, golden, S):
    """Per state count: >= 10 words with bit errors left after the decoder (the label word is the detection), >= 20 whose detected
    bytes differ from the codeword's and still decode to the message (the decoder corrects, the label word is the re-encoding),
    >= 1 without a byte error.  8 ... 128 states: the counts the reference's own words give with the goldens' starting weights."""
    ws = SC.word_set(golden, S)
    clean, corrected, failed = SC.outcomes(golden, S)
    print(f"S={S}: {ws['rx'].shape[0]} words, clean {clean}, corrected {corrected}, failed {failed}")
    assert ws["rx"].shape[0] >= (40 if S == 4 else 50)
    assert clean >= 1 and corrected >= 20 and failed >= 10
    recorded = {8: (7, 33, 10), 32: (1, 25, 24), 64: (3, 26, 21), 128: (1, 33, 16)}
    if S in recorded:
        assert (clean, corrected, failed) == recorded[S]
    dec, ref = SC.detected(golden, S)
    assert np.array_equal(ref["label_word"][ref["nerr"] > 0], dec[ref["nerr"] > 0])
    assert np.array_equal(ref["label_word"][ref["nerr"] == 0], ws["cw"][ref["nerr"] == 0])
    assert ref["labels"].max() == S - 1 and ref["labels"].min() == 0  # the labels are states of THIS trellis


def test_expected_labels_use_the_words_own_memory(oracle):
    """expected_step's labels at 16 states are codec_cases.reference_step's, and differ from them at every other state count."""
    import codec_cases as C

    rng = np.random.RandomState(5)
    msg = rng.randint(0, 2, (3, 120)).astype(np.float32)
    base = C.reference_step(None, msg, 2, True)
    assert np.array_equal(SC.expected_step(None, msg, 2, True, 16)["labels"], base["labels"])
    for S in SC.STATES:
        lab = SC.expected_step(None, msg, 2, True, S)["labels"]
        assert not np.array_equal(lab, base["labels"]) and lab.max() < S
        L = SC.memory(S)
        word = np.concatenate([base["label_word"], np.zeros((3, L), np.float32)], axis=1)
        want = sum((word[:, i:i + 136].astype(np.int32) << i) for i in range(L))
        assert np.array_equal(lab, want)


# ------------------------------------------------------------------------------------------------------------- validation
def call(lib, name="mvn_vnet_byword_step_states_f32", T=136, nsym=2, S=8, R=1, pilot=0, null=(), ld=None):
    """The entry point with every pointer but those in `null` non-NULL (never dereferenced: the case ends before a launch; w_stride,
    which the host would read, is always NULL) and every leading dimension T but those in `ld`."""
    p = {n: None if n in null else ctypes.c_void_p(64) for n in POINTERS}
    lds = dict({n: T for n in ("rx", "tx", "dec", "msg", "enc", "lw", "labels")}, **(ld or {}))
    return getattr(lib, name)(p["rx"], lds["rx"], p["tx"], lds["tx"], *[p[w] for w in WEIGHTS], None, p["dec"], lds["dec"], p["msg"],
                              lds["msg"], p["enc"], lds["enc"], p["lw"], lds["lw"], p["labels"], lds["labels"], p["nerr"], R, T, nsym,
                              pilot, S, None)


def test_max_symbols(lib):
    """min(1024, what the LDS holds): 1024 at 4 and 8 states, >= 512 at 32, >= 256 at 64, >= 136 at 128 (the reference's word,
    120 + 8 * 2); a multiple of 8; 0 for a state count the step does not serve."""
    got = {S: int(lib.mvn_vnet_byword_step_max_symbols(S)) for S in (1, 2, 4, 8, 12, 16, 32, 64, 128, 256, 0, -4)}
    print(got)
    assert got[4] == 1024 and got[8] == 1024
    assert 512 <= got[32] <= 1024 and 256 <= got[64] <= 1024 and 136 <= got[128] <= 1024
    assert all(v % 8 == 0 for v in got.values())
    assert got[16] == 1024  # (the step it forwards to)
    assert all(got[S] == 0 for S in (1, 2, 12, 256, 0, -4))
    for S in SC.STATES:
        assert mvn._lib.step_max_symbols(S) == got[S]


def test_states_step_argument_validation(lib):
    wrong = []

    def expect(code, **case):
        got = call(lib, **case)
        if got != code:
            wrong.append((case, got, code))

    for S in (2, 12, 256):  # the state count first: before the shapes, before R = 0
        expect(-2, S=S, null=ALL)
        expect(-2, S=S, R=0)
        expect(-2, S=S, T=135, R=0)
        expect(-2, S=S, T=135, null=ALL)
    for S in SC.STATES:
        mx = int(lib.mvn_vnet_byword_step_max_symbols(S))
        expect(-1, S=S, T=135, null=ALL)
        expect(-1, S=S, T=135, R=0)
        expect(-1, S=S, nsym=0, null=ALL)
        expect(-1, S=S, nsym=9, null=ALL)
        expect(-1, S=S, T=16, nsym=2, null=ALL)   # T / 8 <= nsym
        expect(-1, S=S, T=64, nsym=8, R=0)
        expect(0, S=S, T=72, nsym=8, R=0)
        expect(-1, S=S, T=mx + 8, null=ALL)
        expect(-1, S=S, T=mx + 8, R=0)
        expect(-1, S=S, R=-1, null=ALL)
        expect(-1, S=S, null=ALL, ld={"rx": 135})
        expect(-1, S=S, R=0, ld={"rx": 135})
        expect(-1, S=S, R=0, ld={"tx": 119})
        for name, short in (("dec", 135), ("msg", 119), ("enc", 135), ("lw", 135), ("labels", 135)):
            expect(-1, S=S, R=0, ld={name: short})
            expect(0, S=S, R=0, ld={name: short}, null=(name,))  # (an output that is not asked for has no leading dimension)
        expect(0, S=S, R=0)
        expect(0, S=S, R=0, null=ALL)  # nothing to do: before any pointer is looked at
        expect(0, S=S, T=mx, R=0)
        expect(-4, S=S, T=mx, null=ALL)
        expect(-4, S=S, null=ALL)
        expect(-4, S=S, null=("rx",))
        expect(-4, S=S, null=("tx",))
        expect(-4, S=S, pilot=1, null=("tx",))
        for w in WEIGHTS:
            expect(-4, S=S, null=(w,))
            expect(-4, S=S, pilot=1, null=(w,))
    assert not wrong, "(case, returned, expected): " + "; ".join(map(repr, wrong))


def test_sixteen_states_forward_to_the_sixteen_state_step(lib):
    """S = 16 through the new entry point: the codes of mvn_vnet_byword_step_f32 for the same arguments."""
    cases = [dict(null=ALL), dict(R=0), dict(T=135, null=ALL), dict(T=1024, R=0), dict(T=1032, R=0), dict(nsym=9, R=0),
             dict(null=("tx",)), dict(pilot=1, null=("rx",), R=0), dict(R=0, ld={"enc": 135}), dict(null=("W3",)), dict(R=-1, null=ALL)]
    for case in cases:
        assert call(lib, S=16, **case) == call(lib, "mvn_vnet_byword_step_f32", S=16, **case), case
    assert call(lib, S=16, null=ALL) == -4 and call(lib, S=16, R=0) == 0 and call(lib, S=16, T=1032, R=0) == -1


# ------------------------------------------------------------------------------------------------------------- the call site
def test_byword_step_resolves_the_states_symbol(lib):
    step = mvn._lib.BywordStep("vnet", "running", 136, 2, n_states=8)
    assert step.name == "mvn_vnet_byword_step_states_f32" and step.n_states == 8
    assert ctypes.cast(step.fn, ctypes.c_void_p).value == ctypes.cast(lib.mvn_vnet_byword_step_states_f32, ctypes.c_void_p).value
    assert mvn._lib.BywordStep("vnet", "running", 136, 2).name == "mvn_vnet_byword_step_f32"
    assert mvn._lib.BywordStep("vnet", "running", 136, 2, n_states=16).name == "mvn_vnet_byword_step_f32"
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("va", "running", 136, 2, n_states=8)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "path", 136, 2, n_states=8)
    with pytest.raises(ValueError):
        mvn._lib.BywordStep("vnet", "list", 136, 2, 4, n_states=8)
