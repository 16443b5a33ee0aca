"""CPU-only: the block step at 4, 8, 32, 64 and 128 states (byword_step_states_kernel<S, NS>, csrc/byword_step_states.inc) exists in
all ten instantiations, uses no scratch, and its static LDS plus the logit image of the longest word it accepts
(mvn_vnet_byword_step_max_symbols) stays within a CU's 160 KB.  Read from the gfx950 code object inside the built libmvn_hip.so, as
tests/test_kernel_resources.py does."""
import re

import meta_viterbinet_amd as mvn
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

STATES = (4, 8, 32, 64, 128)


def test_states_step_kernels_fit_the_cu(resources):  # noqa: F811
    names = sorted(n for n in resources if re.fullmatch(r"byword_step_states_kernel<\d+, \d+>", n))
    assert names == sorted(f"byword_step_states_kernel<{S}, {NS}>" for S in STATES for NS in (2, 8))
    lib = mvn._lib.load()
    for S in STATES:
        max_T = int(lib.mvn_vnet_byword_step_max_symbols(S))
        assert max_T >= 136 and max_T % 8 == 0
        for NS in (2, 8):
            n = f"byword_step_states_kernel<{S}, {NS}>"
            total = resources[n]["lds"] + 4 * S * max_T
            print(n, resources[n], "max symbols", max_T, "LDS at the longest word", total)
            assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
            assert total <= 163840, f"{n}: {total} bytes of LDS at T = {max_T}"
            assert resources[n]["vgpr"] <= 256, f"{n}: {resources[n]['vgpr']} VGPRs, two waves per SIMD leave 256"
