"""CPU-only: the word-axis training kernel (online_train_words_kernel<0 | 16 | 32 | 64 | 128>, csrc/online_train.inc) exists in its
five instantiations, its dynamic LDS stays within a CU's 160 KB at every state count it serves, and it uses no more scratch than its
one-word twin online_train_kernel<SC, false, 1024> is built with (0 bytes at run-time, 16 and 32 states; 8 bytes at 64 and 128).
Read from the gfx950 code object inside the built libmvn_hip.so, as tests/test_kernel_resources.py does."""
import re

import meta_viterbinet_amd as mvn
from test_kernel_resources import resources  # noqa: F401  (the module-scoped fixture that reads the code object)

CU_LDS = 163840
SCRATCH = {0: 0, 16: 0, 32: 0, 64: 8, 128: 8}
SERVES = {0: (2, 4, 8, 32), 16: (16,), 32: (32,), 64: (64,), 128: (128,)}  # the state counts an instantiation runs (plan_train)


def test_word_axis_kernels_fit_the_cu(resources):  # noqa: F811
    names = sorted(n for n in resources if re.fullmatch(r"online_train_words_kernel<\d+>", n))
    assert names == sorted(f"online_train_words_kernel<{SC}>" for SC in SCRATCH)
    lib = mvn._lib.load()
    for SC, scratch in SCRATCH.items():
        n, twin = f"online_train_words_kernel<{SC}>", f"online_train_kernel<{SC}, false, 1024>"
        print(n, resources[n], "twin", resources[twin])
        assert resources[n]["scratch"] <= scratch, f"{n}: {resources[n]['scratch']} bytes of scratch, its one-word twin has {scratch}"
        assert resources[twin]["scratch"] == scratch  # (what the bound was read from)
        assert resources[n]["vgpr"] <= 128, f"{n}: {resources[n]['vgpr']} VGPRs, a 1024-thread workgroup leaves 128"
        for S in SERVES[SC]:
            total = resources[n]["lds"] + int(lib.mvn_vnet_train_lds_bytes(0, S))
            assert 0 < total <= CU_LDS, f"{n}: {total} bytes of LDS at {S} states"
