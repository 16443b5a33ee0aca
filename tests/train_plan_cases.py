"""What mvn_vnet_train_kernel_name answers over one grid of training calls, for tests/test_gpu_train_plan.py.

The answer of a call is the kernel-name string, or `E<code>` where the library refuses the shape (invalid combinations are part
of the grid).  ask(lib) gives {"cus", "answers": [every distinct answer], "tables": {setting: [index into answers, in grid() order]}}:
the recorded tables under tests/golden/ hold what the library gave BEFORE the launchers and the name query were put on one plan
(58 800 answers each, kept as {"cus", "zlib_base64": the JSON text of answers and tables, deflated}: save() / load()).

    python tests/train_plan_cases.py LIBRARY OUT.json      (records a table from a given build of the library)
"""
import base64
import ctypes
import itertools
import json
import os
import sys
import zlib

KINDS = (0, 1, 2)  # online, first-order, second-order meta-learning
TRIALS = (0, 1, 3, 29, 52, 257, 600)  # R (0 = the single-trial entry points)
LENGTHS = (32, 33, 136, 256, 257, 1000, 1056)  # T
WINDOWS = (0, 1, 2, 32)  # M (online) or W (meta-learning)
STATES = (4, 16, 32, 64, 128)
WORKSPACES = ("none", "need", "short", "large")  # 0, the exact need, one byte less, 1 << 26

# the default environment and the three settings of tests/test_gpu_trials.py (FORMS)
SWITCHES = ("MVN_TRAIN_GROUPS", "MVN_TRAIN_PAIR", "MVN_TRAIN_XCD")
SETTINGS = {"default": {}, "chunked": {"MVN_TRAIN_GROUPS": "1", "MVN_TRAIN_PAIR": "0"},
            "per_trial": {"MVN_TRAIN_GROUPS": "0", "MVN_TRAIN_PAIR": "0"}, "pair": {"MVN_TRAIN_GROUPS": "0", "MVN_TRAIN_PAIR": "1"},
            "chunked_spread": {"MVN_TRAIN_GROUPS": "1", "MVN_TRAIN_PAIR": "0", "MVN_TRAIN_XCD": "0"}}


def grid():
    return itertools.product(KINDS, TRIALS, LENGTHS, WINDOWS, STATES, WORKSPACES)


def workspace_bytes(lib, kind, R, T, M_or_W, S, which):
    if which == "none":
        return 0
    if which == "large":
        return 1 << 26
    need = int(lib.mvn_vnet_train_trials_workspace_bytes(S, T, M_or_W if kind else 0, R) if R else lib.mvn_vnet_train_workspace_bytes(S))
    return need if which == "need" else max(need - 1, 0)


def device_cus():
    """CUs of the device the library plans for (0 without a GPU: every shape is then one workgroup per trial)"""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 0


def ask(lib):
    """lib: a loaded build of the library (meta_viterbinet_amd._lib.load() / load_variant()).  Leaves the environment as it was."""
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}
    name = ctypes.create_string_buffer(128)
    answers, tables = {}, {}
    try:
        for setting, env in SETTINGS.items():
            os.environ.update(env)
            lib.mvn_reload_switches()
            table = tables[setting] = []
            for kind, R, T, M_or_W, S, which in grid():
                rc = lib.mvn_vnet_train_kernel_name(kind, R, T, M_or_W, S, workspace_bytes(lib, kind, R, T, M_or_W, S, which), name, 128)
                table.append(answers.setdefault(f"E{rc}" if rc else name.value.decode(), len(answers)))
            for switch in env:
                del os.environ[switch]
    finally:
        for switch, value in saved.items():
            os.environ.pop(switch, None)
            if value is not None:
                os.environ[switch] = value
        lib.mvn_reload_switches()
    return {"cus": device_cus(), "answers": list(answers), "tables": tables}


def first_difference(recorded, got):
    """None, or a line that names the first grid point at which two ask() results differ"""
    for setting in SETTINGS:
        for case, a, b in zip(grid(), recorded["tables"][setting], got["tables"][setting]):
            if recorded["answers"][a] != got["answers"][b]:
                return f"{setting} {case}: recorded {recorded['answers'][a]!r}, the library says {got['answers'][b]!r}"
    return None


def save(path, result):
    text = json.dumps({"answers": result["answers"], "tables": result["tables"]}, separators=(",", ":")).encode()
    blob = base64.b64encode(zlib.compress(text, 9)).decode()
    with open(path, "w") as f:
        json.dump({"cus": result["cus"], "zlib_base64": [blob[i:i + 120] for i in range(0, len(blob), 120)]}, f, indent=0)
        f.write("\n")


def load(path):
    with open(path) as f:
        kept = json.load(f)
    return {"cus": kept["cus"], **json.loads(zlib.decompress(base64.b64decode("".join(kept["zlib_base64"]))))}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import meta_viterbinet_amd as mvn

    result = ask(mvn._lib.load_variant(sys.argv[1]))
    save(sys.argv[2], result)
    print(f"{sys.argv[2]}: {result['cus']} CUs, {len(result['answers'])} distinct answers, {sum(map(len, result['tables'].values()))} calls")
