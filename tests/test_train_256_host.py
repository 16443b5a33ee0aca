"""CPU only: the 256-state online-training kernels (online_train_kernel<256, false> and the word axis'
online_train_words_states256_kernel, csrc/online_train.inc) as far as they can be seen without a device: which entry points accept
256 states and which still refuse them (no case reaches a launch), the kernel the launcher names, the dynamic LDS of the
single-trial online kernels at every state count (mvn_vnet_online_train_lds_bytes) and the two kernels in the gfx950 code object --
their VGPRs within what a 1024-thread workgroup leaves, static + dynamic LDS within a CU, their scratch printed."""
import ctypes

import pytest

import meta_viterbinet_amd as mvn
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

CU_LDS = 163840
OK, E_DIMS, E_STATES, E_NULL = 0, -1, -2, -4
KERNELS = ("online_train_kernel<256, false, 1024>", "online_train_words_states256_kernel")
ADAM = [1e-3, 0.9, 0.999, 1e-8]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


def _online(lib, S, ws, n_iter=1):
    """every pointer NULL: T = 136, M = 32"""
    head = [None, None, 136, None, 32, n_iter] + [None] * 8 + [0] + ADAM + [None, S]
    if ws:
        return lib.mvn_vnet_online_train_ws_f32(*head, None, 0, None, None)
    return lib.mvn_vnet_online_train_f32(*head, None)


def _words(lib, S, n_iter=1):
    """every pointer NULL: two words of 136 symbols, K = 120, M = 32"""
    return lib.mvn_vnet_train_words_states_f32(None, 136, None, 120, 2, 120, None, None, 32, n_iter, *([None] * 8), 0, *ADAM, None, S, None)


def test_single_trial_entry_points_accept_256_states(lib):
    """With the state count accepted, the NULL pointers are what a call stops at (-4); the parent stopped at the state count (-2)."""
    for S in (2, 16, 128, 256):
        assert _online(lib, S, False) == E_NULL and _online(lib, S, True) == E_NULL and _words(lib, S) == E_NULL
        assert _online(lib, S, False, 0) == OK and _online(lib, S, True, 0) == OK and _words(lib, S, 0) == OK
    for S in (0, 48, 512):
        assert _online(lib, S, False) == E_STATES and _online(lib, S, True) == E_STATES and _words(lib, S) == E_STATES
    assert lib.mvn_vnet_online_train_f32(None, None, 0, None, 32, 1, *([None] * 8), 0, *ADAM, None, 256, None) == E_DIMS  # shapes first
    # mvn_vnet_train_words_f32 itself keeps its limit (tests/test_train_words_host.py): the word axis at 256 states is the _states_ call
    old = lambda S, n_iter: lib.mvn_vnet_train_words_f32(None, 136, None, 120, 2, 120, None, None, 32, n_iter, *([None] * 8), 0, *ADAM, None, S, None)  # noqa: E731
    assert old(256, 1) == E_STATES and old(256, 0) == E_STATES and old(128, 1) == E_NULL and old(128, 0) == OK
    assert lib.mvn_vnet_train_words_states_f32(None, 119, None, 120, 2, 120, None, None, 32, 1, *([None] * 8), 0, *ADAM, None, 512, None) == E_DIMS


def test_everything_else_still_refuses_256_states(lib):
    """The trial axis and meta-learning stop at 128 states (32 for the trial-batched meta-learning step)."""
    assert lib.mvn_vnet_online_train_trials_f32(None, 4, 136, 0, *ADAM, 256, None, 0, None) == E_STATES
    assert lib.mvn_vnet_online_train_trials_f32(None, 4, 136, 32, *ADAM, 128, None, 0, None) == E_NULL
    maml = [None, None, 136, None, 1, None, 1] + [None] * 8 + [0, 0.1, 1] + ADAM + [None, 256]
    assert lib.mvn_vnet_maml_train_f32(*maml, None) == E_STATES
    assert lib.mvn_vnet_maml_train_ws_f32(*maml, None, 0, None, None) == E_STATES
    assert lib.mvn_vnet_maml_train_trials_f32(None, 4, 136, 1, 0.1, 1, *ADAM, 256, None, 0, None) == E_STATES
    assert lib.mvn_vnet_maml_train_states_trials_f32(None, 4, 136, 1, 0.1, 1, *ADAM, 256, None) == E_STATES
    assert lib.mvn_vnet_train_workspace_bytes(256) == 0 and lib.mvn_vnet_train_trials_workspace_bytes(256, 136, 1, 4) == 0


def test_kernel_name_at_256_states(lib):
    buf = ctypes.create_string_buffer(160)
    for T, M, ws in ((136, 0, 0), (136, 32, 0), (1, 0, 0), (136, 70, 1 << 22), (1000, 0, 1 << 22)):  # (no workspace form above 32 states)
        assert lib.mvn_vnet_train_kernel_name(0, 0, T, M, 256, ws, buf, 160) == OK
        assert buf.value.decode() == "online_train_kernel<256, false> 1x1"
    for R in (1, 4):
        assert lib.mvn_vnet_train_kernel_name(0, R, 136, 0, 256, 0, buf, 160) == E_STATES
    for kind in (1, 2):
        assert lib.mvn_vnet_train_kernel_name(kind, 0, 136, 1, 256, 0, buf, 160) == E_STATES
        assert lib.mvn_vnet_train_kernel_name(kind, 1, 136, 1, 256, 0, buf, 160) == E_STATES
    assert lib.mvn_vnet_train_kernel_name(0, 0, 136, 0, 512, 0, buf, 160) == E_STATES
    assert lib.mvn_vnet_train_kernel_name(0, 0, 136, 0, 128, 0, buf, 160) == OK and buf.value == b"online_train_kernel<128, false> 1x1"


def test_online_lds_query(lib):
    """Up to 128 states the new query is mvn_vnet_train_lds_bytes(0, S), which stays 0 at 256; at 256: parameters (18 408 floats),
    the gradient vector without dW3 (18 408 - 12 800), the chunk arena with 258-float dlogits rows (15 587) and 64 floats of slack."""
    f, old = lib.mvn_vnet_online_train_lds_bytes, lib.mvn_vnet_train_lds_bytes
    for S in (2, 4, 8, 16, 32, 64, 128):
        assert f(S) == old(0, S) and 0 < f(S) <= CU_LDS, (S, f(S))
    assert all(old(kind, 256) == 0 for kind in (0, 1, 2))
    assert f(256) == 4 * (18408 + (18408 - 12800) + 15587 + 64) == 158668
    for S in (0, 1, 3, 48, 512, -256):
        assert f(S) == 0


def test_kernels_fit_the_workgroup_and_the_cu(lib, resources):  # noqa: F811
    need = int(lib.mvn_vnet_online_train_lds_bytes(256))
    for n in KERNELS:
        assert n in resources, f"{n} is not in the gfx950 code object"
        r = resources[n]
        print(n, r, "dynamic LDS", need, "scratch bytes per thread", r["scratch"], "(the 128-state form: 8)")
        assert r["vgpr"] <= 128, f"{n}: {r['vgpr']} VGPRs, a 1024-thread workgroup leaves 128"
        assert 0 < r["lds"] + need <= CU_LDS, f"{n}: {r['lds'] + need} bytes of LDS"
    assert "online_train_kernel<256, true, 1024>" not in resources and "online_train_words_kernel<256>" not in resources
    assert resources["online_train_kernel<128, false, 1024>"]["scratch"] == 8  # (what the printed figure is compared with)


def test_cpu_and_switched_off_detectors_keep_autograd():
    """words_kernel_route: a CPU detector of 256 states, and use_kernel=False, stay on autograd."""
    det = mvn.VNETDetector(256, {"train": 8, "val": 8}).to("cpu")
    assert not mvn.OnlineTrainer(det, 8).words_kernel_route() and not mvn.OnlineTrainer(det, 8, use_kernel=False).words_kernel_route()
