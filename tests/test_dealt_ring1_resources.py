"""CPU-only: the dealt kernel's ring-of-one form (vnet16_dealt_ring1_kernel, csrc/vnet16_dealt.inc) is built for 6 waves per SIMD
like the general form: at most 80 VGPRs, no scratch, and no more LDS than the general form (3 workgroups per CU).  Read from the
gfx950 code object inside the built libmvn_hip.so, as tests/test_kernel_resources.py does."""
import re

from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)


def test_ring1_kernels_keep_six_waves_per_simd(resources):  # noqa: F811
    names = [n for n in resources if re.fullmatch(r"vnet16_dealt_ring1_kernel<(false|true)>", n)]
    assert sorted(names) == ["vnet16_dealt_ring1_kernel<false>", "vnet16_dealt_ring1_kernel<true>"]
    general = resources["vnet16_dealt_kernel<false, false>"]
    for n in names:
        print(n, resources[n])
        assert resources[n]["vgpr"] <= 80, f"{n}: {resources[n]['vgpr']} VGPRs, built for <= 80"
        assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
        assert resources[n]["lds"] <= general["lds"], f"{n}: {resources[n]['lds']} bytes of LDS, the general form {general['lds']}"
