"""CPU only: the trial axis of the meta-learning step at 64 and 128 states (mvn_vnet_maml_train_states_trials_f32,
maml_train_states_trials_kernel<64 | 128>, csrc/maml_train.inc) as far as it can be seen without a device: the symbol and its
signature, the entry point's argument validation in its documented order (no case reaches a launch), the two instantiations in the
gfx950 code object with their registers, the routing predicates of trials.py and the validation of meta_trial_axis."""
import re

import pytest

import meta_viterbinet_amd as mvn
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

OK, E_DIMS, E_STATES, E_NULL = 0, -1, -2, -4
ENTRY = "mvn_vnet_maml_train_states_trials_f32"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


def _call(lib, S=64, R=4, T=136, W=1, beta1=0.9):
    """a call with the descriptor array NULL: second order, meta_lr 0.1, Adam's usual constants"""
    return getattr(lib, ENTRY)(None, R, T, W, 0.1, 1, 1e-3, beta1, 0.999, 1e-8, S, None)


def test_symbol_and_signature(lib):
    assert ENTRY in mvn._lib.SIGNATURES
    restype, argtypes = mvn._lib.SIGNATURES[ENTRY]
    sibling = mvn._lib.SIGNATURES["mvn_vnet_maml_train_trials_f32"]
    assert restype is sibling[0]
    assert argtypes == sibling[1][:11] + sibling[1][13:]  # the sibling's arguments without (workspace, workspace_bytes)
    assert len(argtypes) == 12
    assert hasattr(lib, ENTRY)


def test_return_codes_in_order(lib):
    for S in (64, 128):
        assert _call(lib, S=S, R=4) == E_NULL
        assert _call(lib, S=S, R=0) == OK
    for S in (16, 32, 256):
        assert _call(lib, S=S) == E_STATES
        assert _call(lib, S=S, R=0) == E_STATES  # the state count is checked before R == 0
    for S in (64, 128, 16, 256):  # the dimensions are checked before the state count
        assert _call(lib, S=S, W=0) == E_DIMS
        assert _call(lib, S=S, T=0) == E_DIMS
        assert _call(lib, S=S, R=-1) == E_DIMS
        assert _call(lib, S=S, beta1=-1.0) == E_DIMS  # RMSprop's tag: Adam only
        assert _call(lib, S=S, beta1=-2.0) == E_DIMS  # SGD's
        assert _call(lib, S=S, R=0, beta1=-1.0) == E_DIMS


def test_existing_entry_points_keep_their_answers(lib):
    import ctypes

    assert lib.mvn_vnet_maml_train_trials_f32(None, 1, 136, 1, 0.1, 1, 1e-3, 0.9, 0.999, 1e-8, 64, None, 0, None) == E_STATES
    assert lib.mvn_vnet_maml_train_trials_f32(None, 1, 136, 1, 0.1, 1, 1e-3, -1.0, 0.999, 1e-8, 16, None, 0, None) == E_DIMS
    assert lib.mvn_vnet_train_trials_workspace_bytes(64, 136, 1, 4) == 0 and lib.mvn_vnet_train_trials_workspace_bytes(128, 136, 2, 300) == 0
    assert lib.mvn_vnet_train_workspace_bytes(64) == 0 and lib.mvn_vnet_train_workspace_bytes(128) == 0
    buf = ctypes.create_string_buffer(160)
    for kind in (1, 2):
        for S in (64, 128):
            assert lib.mvn_vnet_train_kernel_name(kind, 3, 136, 1, S, 0, buf, 160) == E_STATES


def test_instantiations(resources):  # noqa: F811
    """Both instantiations are in the code object; a 1024-thread workgroup leaves each wave 128 VGPRs, above which the kernel cannot
    launch.  Printed beside the one-trial forms (the same body with the descriptor as a kernel argument)."""
    for S in (64, 128):
        one, many = f"maml_train_kernel<{S}, false>", f"maml_train_states_trials_kernel<{S}>"
        assert many in resources, sorted(n for n in resources if "maml_train" in n)
        print(f"{many}: {resources[many]}   |   {one}: {resources[one]}")
        assert resources[many]["vgpr"] <= 128, f"{many}: {resources[many]['vgpr']} VGPRs, 16 waves on a CU leave 128"
        assert resources[many]["lds"] == 0  # all of its LDS is dynamic: mvn_vnet_train_lds_bytes(1, S)
    assert sorted(n for n in resources if re.match(r"maml_train_states_trials_kernel<", n)) == [
        "maml_train_states_trials_kernel<128>", "maml_train_states_trials_kernel<64>"]


# ------------------------------------------------------------------------------------------------------------- routing
class _Cuda:
    """What the predicates look at of the received words: a shape and is_cuda."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape


class _Host(_Cuda):
    is_cuda = False


def test_meta_states_predicate(lib):
    from meta_viterbinet_amd.trials import META_STATES, META_TRIAL_AXIS_MIN_R, _lock_step_serves, _meta_states_serves

    assert META_STATES == (64, 128) and META_TRIAL_AXIS_MIN_R >= 2
    T = 136
    for S in (64, 128):
        long = mvn._lib.step_max_symbols(S) + 8
        for decision in ("running", "path"):
            assert _meta_states_serves(S, _Cuda(3, 50, T), 2, decision, True)
            assert _meta_states_serves(S, _Cuda(1, 50, T), 2, decision, True)  # (R is eval_by_word_batched's business)
            assert _meta_states_serves(S, _Cuda(3, 50, T), 8, decision, True)
            assert _meta_states_serves(S, _Cuda(3, 50, long - 8), 2, decision, True)
            assert not _meta_states_serves(S, _Cuda(3, 50, T), 2, decision, False)  # nothing for it to do without online_meta
            assert not _meta_states_serves(S, _Cuda(3, 50, long), 2, decision, True)  # a word the block step cannot hold
            assert not _meta_states_serves(S, _Cuda(3, 50, T + 4), 2, decision, True)  # T not a multiple of 8
            assert not _meta_states_serves(S, _Cuda(3, 50, T), 0, decision, True)
            assert not _meta_states_serves(S, _Cuda(3, 50, T), 9, decision, True)
            assert not _meta_states_serves(S, _Cuda(3, 50, 16), 2, decision, True)  # no message bytes left
            assert not _meta_states_serves(S, _Host(3, 50, T), 2, decision, True)
            for opt in ("RMSprop", "SGD"):
                assert not _meta_states_serves(S, _Cuda(3, 50, T), 2, decision, True, opt)
            assert _meta_states_serves(S, _Cuda(3, 50, T), 2, decision, True, "Adam")
        assert not _meta_states_serves(S, _Cuda(3, 50, T), 2, "list", True)
    for S in (4, 8, 16, 32, 256):
        for decision in ("running", "path"):
            assert not _meta_states_serves(S, _Cuda(3, 50, T), 2, decision, True)
    # _lock_step_serves is what it was
    for S in (4, 8, 32, 64, 128):
        for decision in ("running", "path"):
            assert _lock_step_serves(S, _Cuda(3, 50, T), 2, decision, False)
            assert _lock_step_serves(S, _Cuda(3, 50, T), 2, decision, True) == (S <= 32)
        assert not _lock_step_serves(S, _Cuda(3, 50, T), 2, "list", False)
    assert _lock_step_serves(16, _Cuda(3, 50, T), 2, "list", True)
    assert not _lock_step_serves(256, _Cuda(3, 50, T), 2, "running", False)


class _NoDevice:
    """A bank / tensor stand-in any use of which fails: the keyword is validated before anything is touched."""

    def __getattr__(self, name):
        raise AssertionError(f"eval_by_word_batched touched .{name} before validating meta_trial_axis")


@pytest.mark.parametrize("bad", [2, 0, 1, "yes", "None", 1.0, [], object()])
def test_meta_trial_axis_is_validated_first(bad):
    from meta_viterbinet_amd.trials import eval_by_word_batched

    with pytest.raises(ValueError, match="meta_trial_axis"):
        eval_by_word_batched(_NoDevice(), _NoDevice(), _NoDevice(), 2, 25, [], online_meta=True, meta_trial_axis=bad)


def test_meta_trial_axis_accepts_none_true_false():
    """The three legal values get past the keyword's check (and fail later, on the stand-in bank)."""
    from meta_viterbinet_amd.trials import eval_by_word_batched

    for good in (None, True, False):
        with pytest.raises(AssertionError, match="touched"):
            eval_by_word_batched(_NoDevice(), _NoDevice(), _NoDevice(), 2, 25, [], online_meta=True, meta_trial_axis=good)
