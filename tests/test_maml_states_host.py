"""CPU only: the meta-learning kernel at 64 and 128 states (maml_train_kernel<64 | 128, false>, csrc/maml_train.inc) as far as it can
be seen without a device: the entry points' argument validation (no case reaches a launch), the kernel the launcher names, the
dynamic LDS of the single-workgroup training launches (mvn_vnet_train_lds_bytes) and the instantiations in the gfx950 code object."""
import ctypes
import re

import pytest

import meta_viterbinet_amd as mvn
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

CU_LDS = 163840
OK, E_DIMS, E_STATES, E_NULL = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


def _maml(lib, S, ws, n_steps=1, beta1=0.9):
    """a call with every pointer NULL: T = 136, W = 1, second order"""
    head = [None, None, 136, None, 1, None, n_steps] + [None] * 8 + [0, 0.1, 1, 1e-3, beta1, 0.999, 1e-8, None, S]
    if ws:
        return lib.mvn_vnet_maml_train_ws_f32(*head, None, 0, None, None)
    return lib.mvn_vnet_maml_train_f32(*head, None)


@pytest.mark.parametrize("ws", [False, True], ids=["maml_train", "maml_train_ws"])
@pytest.mark.parametrize("S", [64, 128])
def test_entry_points_accept_64_and_128_states(lib, S, ws):
    """With the state count accepted, the NULL pointers are what the call stops at (-4); the parent stopped at the state count (-2)."""
    assert _maml(lib, S, ws) == E_NULL


@pytest.mark.parametrize("ws", [False, True], ids=["maml_train", "maml_train_ws"])
def test_other_return_codes(lib, ws):
    for S in (64, 128):
        assert _maml(lib, S, ws, n_steps=0) == OK
        assert _maml(lib, S, ws, beta1=-1.0) == E_DIMS  # RMSprop / SGD: Adam only
    assert _maml(lib, 256, ws) == E_STATES
    assert _maml(lib, 16, ws) == E_NULL


def test_trials_entry_stays_at_32_states(lib):
    assert lib.mvn_vnet_maml_train_trials_f32(None, 1, 136, 1, 0.1, 1, 1e-3, 0.9, 0.999, 1e-8, 64, None, 0, None) == E_STATES
    assert lib.mvn_vnet_maml_train_trials_f32(None, 1, 136, 1, 0.1, 1, 1e-3, 0.9, 0.999, 1e-8, 32, None, 0, None) == E_NULL
    assert lib.mvn_vnet_train_trials_workspace_bytes(64, 136, 1, 4) == 0
    assert lib.mvn_vnet_train_workspace_bytes(64) == 0 and lib.mvn_vnet_train_workspace_bytes(128) == 0  # theta waits in the weights


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("kind", [1, 2])
def test_kernel_name(lib, kind, S):
    buf = ctypes.create_string_buffer(160)
    for ws_bytes in (0, 1 << 30):
        assert lib.mvn_vnet_train_kernel_name(kind, 0, 136, 1, S, ws_bytes, buf, 160) == OK
        assert buf.value.decode() == f"maml_train_kernel<{S}, false> 1x1"
        assert lib.mvn_vnet_train_kernel_name(kind, 0, 136, 2, S, ws_bytes, buf, 160) == OK  # (W = 2: nine chunks, still one workgroup)
        assert buf.value.decode() == f"maml_train_kernel<{S}, false> 1x1"
    assert lib.mvn_vnet_train_kernel_name(kind, 1, 136, 1, S, 0, buf, 160) == E_STATES
    assert lib.mvn_vnet_train_kernel_name(kind, 0, 136, 1, 256, 0, buf, 160) == E_STATES


# maml_train_lds_floats(S) * 4 of the parent commit: 3 P4 + max(P4 + ChunkArena<32>, HvArena<32>) + 64 floats, P4 = 5350 + 51 S
# padded to 4, ChunkArena<32> = 8419, HvArena<32> = 17280
PARENT_MAML_LDS = {2: 134800, 4: 136048, 8: 138496, 16: 143392, 32: 153184}


def test_train_lds_bytes(lib):
    f = lib.mvn_vnet_train_lds_bytes
    for kind in (0, 1, 2):
        for S in (2, 4, 8, 16, 32, 64, 128):
            assert 0 < f(kind, S) <= CU_LDS, (kind, S, f(kind, S))
        assert f(kind, 256) == 0 and f(kind, 48) == 0
    assert f(3, 16) == 0 and f(-1, 16) == 0
    for S, want in PARENT_MAML_LDS.items():
        assert f(1, S) == want and f(2, S) == want
    # two parameter vectors of 5350 + 51 S floats (padded to 4), the 16-row Hessian arena 16 (438 + 3 (S + 2)) -- larger than the
    # gradient passes' 32 (212 + S) + 611 -- and 64 floats of slack
    assert f(1, 64) == f(2, 64) == 4 * (2 * 8616 + 16 * (438 + 3 * 66) + 64) == 109888
    assert f(1, 128) == f(2, 128) == 4 * (2 * 11880 + 16 * (438 + 3 * 130) + 64) == 148288
    print("dynamic LDS:", {(k, S): f(k, S) for k in (0, 1) for S in (32, 64, 128)})


def test_instantiations(resources):  # noqa: F811
    for S in (64, 128):
        assert f"maml_train_kernel<{S}, false>" in resources
    unwanted = [n for n in resources if re.match(r"maml_train_kernel<(64|128), true>|maml_train_groups_kernel<(64|128)\b", n)]
    assert not unwanted, unwanted
    for n in ("maml_train_kernel<32, false>", "maml_train_kernel<64, false>", "maml_train_kernel<128, false>"):
        print(n, resources[n])
        assert resources[n]["vgpr"] <= 128, f"{n}: 16 waves on a CU leave 128 VGPRs"
