"""CPU-only: register and scratch budgets of the kernels that instantiate the shared 16-state ViterbiNet unit
(csrc/vnet16_common.inc), read from the gfx950 code object inside the built libmvn_hip.so.

The kernels built for 80 VGPRs (6 waves per SIMD) keep to them without scratch only in the form the shared code has today
(how the sigmoid reaches the k-loop, opaque lane ids: see the comments there); a compiler update or an edit can tip them over
without any result changing.  The bounds are those of each kernel's __launch_bounds__ (VGPRs per occupancy step on gfx950:
6 waves per SIMD <= 80, 5 <= 96, 4 <= 128), not what today's build happens to use."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

# kernel name pattern -> VGPR budget of the occupancy step it is built for
BUDGETS = [
    (r"vnet16_dealt_kernel<(false|true), false>", 80),
    (r"vnet16_dealt_kernel<false, true>", 96),
    (r"vnet16_fusedn_kernel<(false|true), 2>", 80),
    (r"vnet16_fusedn_kernel<(false|true), 4>", 128),
    (r"vnet16_coop_kernel<(false|true)>", 128),
    (r"byword_step_kernel<(2|8)>", 128),
]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    import __graft_entry__ as g

    so = g.build_hip()
    bundler, readelf = os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")
    assert os.path.exists(bundler) and os.path.exists(readelf), "the ROCm LLVM tools that built the library are missing"
    assert shutil.which("c++filt"), "c++filt is missing"
    tmp = tmp_path_factory.mktemp("co")
    fatbin, elf = str(tmp / "fatbin"), str(tmp / "dev.elf")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, so, str(tmp / "unused")], check=True)
    subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fatbin, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--output=" + elf], check=True)
    notes = subprocess.run([readelf, "--notes", elf], check=True, capture_output=True, text=True).stdout
    table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], input=notes, check=True,
                           capture_output=True, text=True).stdout
    rows = {}
    for line in table.splitlines():
        m = re.match(r"(.+?)\s+vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) static_lds (\d+)$", line)
        if m:
            rows[m.group(1)] = {"vgpr": int(m.group(2)), "scratch": int(m.group(4)), "lds": int(m.group(5))}
    return rows


def test_shared_unit_kernels_keep_their_occupancy_step(resources):
    for pattern, budget in BUDGETS:
        names = [n for n in resources if re.fullmatch(pattern, n)]
        assert names, f"no kernel matches {pattern}"
        for n in names:
            print(n, resources[n])
            assert resources[n]["vgpr"] <= budget, f"{n}: {resources[n]['vgpr']} VGPRs, built for <= {budget}"


def test_fused_detector_kernels_use_no_scratch(resources):
    names = [n for n in resources if re.match(r"(vnet16_|byword_step_kernel|vnet_fused_ip_kernel)", n)]
    assert len(names) >= 17
    for n in names:
        assert resources[n]["scratch"] == 0, f"{n}: {resources[n]['scratch']} bytes of scratch"
