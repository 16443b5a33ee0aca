"""mvn_vnet_train_kernel_name over the grid of tests/train_plan_cases.py against the tables recorded from the library as it
was before plan_train (csrc/mvn_hip.hip): the launchers' one plan decides form, groups, state constant, trials per launch and
grid exactly as the two launchers, the two plan functions and the hand-kept name query did.  No kernel is launched."""
import os

import pytest

import meta_viterbinet_amd as mvn
import train_plan_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check(recorded_file):
    recorded = cases.load(os.path.join(GOLDEN, recorded_file))
    lib = mvn._lib.load()
    cus = cases.device_cus()
    if cus != recorded["cus"]:
        pytest.skip(f"{recorded_file} was recorded at {recorded['cus']} CUs, this device has {cus}")
    got = cases.ask(lib)
    assert {s: len(t) for s, t in got["tables"].items()} == {s: len(t) for s, t in recorded["tables"].items()}
    assert cases.first_difference(recorded, got) is None


@pytest.mark.gpu
def test_train_plan_names_on_the_device():
    """The table recorded on an MI355X (256 CUs): chunked, per-trial and pair forms, both grids, several launches."""
    _check("train_plan_names.json")


def test_train_plan_names_without_a_device():
    """The table recorded without a GPU (0 CUs: every shape is one workgroup per trial); skips where a device is visible."""
    _check("train_plan_names_no_gpu.json")
