"""CPU-only: mvn_vnet_montecarlo_f32 (the 16-state ViterbiNet Monte-Carlo point with the words generated inside the detector,
csrc/vnet_montecarlo.inc) checks its arguments before it touches a device, and vnet16_mc_kernel keeps the resources it is built for.

Every return-code case has B = 0, n_rounds = 0, a bad shape or a NULL pointer, so nothing is launched: the non-NULL pointers are
addresses of host bytes that the library must never read.  The resources are read from the gfx950 code object inside the built
libmvn_hip.so by the fixture of tests/test_kernel_resources.py."""
import ctypes
import os
import re

import pytest

from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_DIMS, E_STATES, E_NULL = 0, -1, -2, -4

# VGPRs per occupancy step on gfx950 (waves per SIMD -> budget), the table of tests/test_kernel_resources.py
VGPR_STEP = {6: 80, 5: 96, 4: 128}
CU_LDS_BYTES = 163840


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    import meta_viterbinet_amd as mvn

    return mvn._lib.load()


_HOST = ctypes.create_string_buffer(64)
P = ctypes.c_void_p(ctypes.addressof(_HOST))  # "some pointer": never dereferenced by a call that returns before its launch


def call(lib, h=P, Bh=1, word0=0, w=(P,) * 6, counters=P, progress=P, B=4, n_rounds=1, F=0, T=100, L=4, S=16):
    return lib.mvn_vnet_montecarlo_f32(h, Bh, 0.25, 7, word0, *w, counters, progress, B, n_rounds, F, T, L, S, None)


def test_states_other_than_16_are_refused_first(lib):
    for S, L in ((2, 1), (4, 2), (8, 3), (32, 5), (64, 6), (256, 8), (12, 4), (0, 0)):
        assert call(lib, S=S, L=L, B=0) == E_STATES, (S, L)
        assert call(lib, S=S, L=L, h=None, T=0, Bh=0) == E_STATES, (S, L)  # before the shapes and the pointers


def test_shapes_come_before_pointers(lib):
    none = dict(h=None, w=(None,) * 6, counters=None, progress=None)
    for bad in (dict(L=3), dict(L=5), dict(L=-1), dict(L=40), dict(T=0), dict(T=-5), dict(B=-1), dict(n_rounds=-1), dict(Bh=0), dict(Bh=-2),
                dict(word0=-1), dict(F=-1)):
        assert call(lib, **bad, **none) == E_DIMS, bad
        assert call(lib, **{**dict(B=0), **bad}) == E_DIMS, bad  # a bad shape is an error even where there is nothing to do


def test_nothing_to_do_is_ok_without_pointers(lib):
    none = dict(h=None, w=(None,) * 6, counters=None, progress=None)
    assert call(lib, B=0, **none) == OK
    assert call(lib, n_rounds=0, **none) == OK
    assert call(lib, B=0, n_rounds=12, F=5, **none) == OK


def test_null_pointers_with_work_to_do(lib):
    assert call(lib, h=None) == E_NULL
    assert call(lib, counters=None) == E_NULL
    for i in range(6):
        w = [P] * 6
        w[i] = None
        assert call(lib, w=tuple(w)) == E_NULL, f"weight array {i}"
    # the progress array: needed by the gate between rounds, so with more than one round or a stop rule
    assert call(lib, progress=None, n_rounds=2, h=None) == E_NULL
    assert call(lib, progress=None, n_rounds=2) == E_NULL
    assert call(lib, progress=None, n_rounds=1, F=3) == E_NULL


def test_binding_and_version(lib):
    import meta_viterbinet_amd as mvn

    assert lib.mvn_version() == 6
    assert "mvn_vnet_montecarlo_f32" in mvn._lib.SIGNATURES and "vnet_monte_carlo" in mvn.__all__
    with pytest.raises(mvn._lib.MvnError):
        mvn.vnet_monte_carlo(None, 1, None, 10.0, "cpu", 1)  # no host fall-back


def _built_for():
    """(waves per workgroup, workgroups per CU) that vnet16_mc_kernel's __launch_bounds__ ask for: the fused detector's defaults in
    csrc/vnet16_fusedn.inc, which the Monte-Carlo kernel shares."""
    text = open(os.path.join(ROOT, "meta-viterbinet_amd", "csrc", "vnet16_fusedn.inc")).read()
    waves = int(re.search(r"#define MVN_FN_WAVES (\d+)", text).group(1))
    wgs = int(re.search(r"#define MVN_FN_WGS (\d+)", text).group(1))
    mc = open(os.path.join(ROOT, "meta-viterbinet_amd", "csrc", "vnet_montecarlo.inc")).read()
    assert re.search(r"__launch_bounds__\(64 \* kFusedNWaves, FusedNCfg<2>::kMinWgPerCu\)\s+void vnet16_mc_kernel", mc)
    return waves, wgs


def test_mc_kernel_resources(resources):  # noqa: F811
    assert "vnet16_mc_kernel" in resources, sorted(n for n in resources if "mc" in n)
    r = resources["vnet16_mc_kernel"]
    waves, wgs = _built_for()
    per_simd = (waves * wgs + 3) // 4  # FusedNCfg<2>::kMinWgPerCu
    print("vnet16_mc_kernel", r, "built for", wgs, "workgroups of", waves, "waves per CU =", per_simd, "waves per SIMD")
    assert r["scratch"] == 0, f"{r['scratch']} bytes of scratch"
    assert r["vgpr"] <= VGPR_STEP[per_simd], f"{r['vgpr']} VGPRs, built for <= {VGPR_STEP[per_simd]} ({per_simd} waves per SIMD)"
    assert r["lds"] * wgs <= CU_LDS_BYTES, f"{wgs} workgroups x {r['lds']} bytes of LDS exceed a CU's {CU_LDS_BYTES}"
    # the weights' image, the scratch image and the lane table of the fused detector + 1280 bytes per wave of samples and bits
    assert r["lds"] >= resources["vnet16_fusedn_kernel<false, 2>"]["lds"] + waves * (256 * 4 + 64 * 4)
    assert resources["vnet_mc_gate_kernel"]["scratch"] == 0
