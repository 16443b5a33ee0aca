"""CPU only: argument validation of the six by-word block steps (mvn_{vnet,va}_byword_step[_path|_list]_f32), one table over all of
them.  No case reaches a launch: each has R = 0 or a required pointer NULL, so no device is touched.  The expected codes of the cases
that test_abi.py, test_path_step_host.py and test_list_step_host.py held before this table are theirs; the codes of the others were
recorded from the library as it was before the entry points were put on one shared check (its build loaded through MVN_LIB_PATH),
never from the code under test."""
import ctypes

import pytest

import meta_viterbinet_amd as mvn

ENTRIES = [("vnet", "running"), ("va", "running"), ("vnet", "path"), ("va", "path"), ("vnet", "list"), ("va", "list")]
SUFFIX = {"running": "_f32", "path": "_path_f32", "list": "_list_f32"}
WEIGHTS = ("W1", "b1", "W2", "b2", "W3", "b3")
POINTERS = ("rx", "tx", "priors", "dec", "msg", "enc", "lw", "labels", "nerr", "delta", "choice") + WEIGHTS
ALL = POINTERS


def call(lib, kind, variant, T=136, nsym=2, S=16, R=1, pilot=0, m=4, Bp=1, null=(), ld=None):
    """The entry point with every pointer but those in `null` non-NULL (never dereferenced: the case ends before a launch; w_stride,
    which the host would read, is always NULL) and every leading dimension T but those in `ld`."""
    p = {name: None if name in null else ctypes.c_void_p(64) for name in POINTERS}
    lds = dict({name: T for name in ("rx", "tx", "dec", "msg", "enc", "lw", "labels", "delta")}, **(ld or {}))
    front = (p["priors"], Bp) if kind == "va" else (*[p[w] for w in WEIGHTS], None)
    tail = (m, p["delta"], lds["delta"], p["choice"]) if variant == "list" else ()
    return getattr(lib, f"mvn_{kind}_byword_step{SUFFIX[variant]}")(
        p["rx"], lds["rx"], p["tx"], lds["tx"], *front, p["dec"], lds["dec"], p["msg"], lds["msg"], p["enc"], lds["enc"], p["lw"], lds["lw"],
        p["labels"], lds["labels"], p["nerr"], R, T, nsym, pilot, S, *tail, None)


def ends_before_a_launch(kind, variant, case):
    """Nothing to do, or a pointer this entry point requires is NULL (a code of None in the table: the case is not for this entry)."""
    null, pilot = case.get("null", ()), case.get("pilot", 0)
    no_tx = "tx" in null and (variant != "list" or pilot or not {"nerr", "lw", "labels"} <= set(null))
    no_front = any(w in null for w in WEIGHTS) if kind == "vnet" else ("priors" in null and not pilot)
    return case.get("R", 1) == 0 or ("rx" in null and not pilot) or no_tx or no_front


# What this table cannot show on the CPU: that the list data step ACCEPTS tx == NULL when nothing is compared with it.  Such a case has to
# end before a launch as well, so it also has rx NULL (-4) or R = 0, and a refusal of tx would give the same codes; the acceptance rests
# on tests/test_gpu_list_step.py::test_list_step_with_some_outputs_only (its no_tx cases) alone.
# (case, expected codes in the order of ENTRIES): 0 ok, -1 MVN_E_DIMS, -2 MVN_E_STATES, -3 MVN_E_PRIORS, -4 MVN_E_NULL
CASES = [
    ({'S': 8, 'null': ALL}, (-2, -2, -2, -2, -2, -2)),
    ({'S': 256, 'null': ALL}, (-2, -2, -2, -2, -2, -2)),
    ({'T': 135, 'nsym': 2, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 136, 'nsym': 9, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 16, 'nsym': 2, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 2048, 'nsym': 2, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'null': ALL, 'ld': {'rx': 100}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'null': ALL}, (0, 0, 0, 0, 0, 0)),
    ({'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'Bp': 0, 'null': ALL}, (-4, -3, -4, -3, -4, -3)),
    ({'T': 520, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'T': 1024, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'T': 512, 'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'T': 136, 'nsym': 9, 'm': 9, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'m': 12, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'m': 1, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'m': 18, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'m': 11, 'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'nsym': 1, 'm': 17, 'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'T': 512, 'nsym': 1, 'm': 64, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'T': 128, 'nsym': 8, 'm': 9, 'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'T': 128, 'nsym': 8, 'm': 10, 'null': ALL}, (-4, -4, -4, -4, -4, -4)),
    ({'T': 128, 'nsym': 8, 'm': 11, 'null': ALL}, (-4, -4, -4, -4, -1, -1)),
    ({'S': 8, 'R': 0}, (-2, -2, -2, -2, -2, -2)),
    ({'S': 256, 'R': 0}, (-2, -2, -2, -2, -2, -2)),
    ({'S': 8, 'T': 135, 'R': 0}, (-2, -2, -2, -2, -2, -2)),
    ({'S': 8, 'Bp': 0, 'R': 0}, (-2, -2, -2, -2, -2, -2)),
    ({'R': -1, 'null': ALL}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 0, 'nsym': 1, 'm': 1, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 135, 'nsym': 2, 'm': 2, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 1032, 'nsym': 2, 'm': 2, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 1024, 'nsym': 2, 'm': 2, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 136, 'nsym': 0, 'm': 1, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 136, 'nsym': 9, 'm': 9, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 16, 'nsym': 2, 'm': 2, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 64, 'nsym': 8, 'm': 8, 'R': 0}, (-1, -1, -1, -1, -1, -1)),
    ({'T': 72, 'nsym': 8, 'm': 8, 'R': 0}, (0, 0, 0, 0, 0, 0)),
    ({'T': 520, 'nsym': 2, 'm': 4, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 136, 'nsym': 2, 'm': 1, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 136, 'nsym': 2, 'm': 18, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 136, 'nsym': 2, 'm': 12, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 136, 'nsym': 2, 'm': 11, 'R': 0}, (0, 0, 0, 0, 0, 0)),
    ({'T': 512, 'nsym': 1, 'm': 64, 'R': 0}, (0, 0, 0, 0, -1, -1)),
    ({'T': 512, 'nsym': 1, 'm': 63, 'R': 0}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'rx': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'rx': 135}, 'null': ('rx',)}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'rx': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'tx': 119}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'tx': 119}, 'null': ('tx',)}, (-1, -1, -1, -1, 0, 0)),
    ({'R': 0, 'ld': {'tx': 120}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'dec': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'dec': 135}, 'null': ('dec',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'dec': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'msg': 119}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'msg': 119}, 'null': ('msg',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'msg': 120}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'enc': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'enc': 135}, 'null': ('enc',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'enc': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'lw': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'lw': 135}, 'null': ('lw',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'lw': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'labels': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'ld': {'labels': 135}, 'null': ('labels',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'labels': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'delta': 135}}, (0, 0, 0, 0, -1, -1)),
    ({'R': 0, 'ld': {'delta': 135}, 'null': ('delta',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'ld': {'delta': 136}}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'pilot': 1, 'ld': {'tx': 119}, 'null': ('tx',)}, (-1, -1, -1, -1, -1, -1)),
    ({'R': 0, 'pilot': 1, 'ld': {'delta': 135}}, (0, 0, 0, 0, -1, -1)),
    ({'R': 0, 'pilot': 1, 'm': 12}, (0, 0, 0, 0, -1, -1)),
    ({'Bp': 0, 'R': 0}, (0, -3, 0, -3, 0, -3)),
    ({'Bp': 0, 'R': 0, 'ld': {'enc': 135}}, (-1, -1, -1, -1, -1, -1)),
    ({'Bp': -1, 'R': 0, 'pilot': 1}, (0, -3, 0, -3, 0, -3)),
    ({'Bp': 0, 'R': 1, 'null': ALL}, (-4, -3, -4, -3, -4, -3)),
    ({'null': ('rx',)}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx',)}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('priors',)}, (None, -4, None, -4, None, -4)),
    ({'null': ('W1',)}, (-4, None, -4, None, -4, None)),
    ({'null': ('b1',)}, (-4, None, -4, None, -4, None)),
    ({'null': ('W2',)}, (-4, None, -4, None, -4, None)),
    ({'null': ('b2',)}, (-4, None, -4, None, -4, None)),
    ({'null': ('W3',)}, (-4, None, -4, None, -4, None)),
    ({'null': ('b3',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('rx', 'tx')}, (-4, -4, -4, -4, -4, -4)),
    ({'pilot': 1, 'null': ('tx',)}, (-4, -4, -4, -4, -4, -4)),
    ({'pilot': 1, 'null': ('priors', 'tx')}, (-4, -4, -4, -4, -4, -4)),
    ({'pilot': 1, 'null': ('W1',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('b1',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('W2',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('b2',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('W3',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'null': ('b3',)}, (-4, None, -4, None, -4, None)),
    ({'pilot': 1, 'R': 0, 'null': ('rx', 'priors')}, (0, 0, 0, 0, 0, 0)),
    ({'null': ('tx', 'rx')}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx', 'rx', 'nerr')}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx', 'rx', 'nerr', 'lw')}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx', 'rx', 'nerr', 'lw', 'labels')}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx', 'nerr', 'labels')}, (-4, -4, -4, -4, -4, -4)),
    ({'null': ('tx', 'nerr', 'lw')}, (-4, -4, -4, -4, -4, -4)),
    ({'R': 0, 'null': ('tx', 'nerr', 'lw', 'labels')}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'null': ('tx',)}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0}, (0, 0, 0, 0, 0, 0)),
    ({'R': 0, 'T': 1024, 'nsym': 8, 'm': 8}, (0, 0, 0, 0, -1, -1)),
]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build_hip()
    return mvn._lib.load()


def test_step_argument_validation(lib):
    assert lib.mvn_version() == 6
    wrong = []
    for case, codes in CASES:
        for (kind, variant), code in zip(ENTRIES, codes):
            if code is not None:
                assert ends_before_a_launch(kind, variant, case), (case, kind, variant)
                got = call(lib, kind, variant, **case)
                if got != code:
                    wrong.append((case, kind, variant, got, code))
    assert not wrong, "(case, kind, variant, returned, expected): " + "; ".join(map(repr, wrong))
    assert len(CASES) >= 100 and all(any(c is not None for c in codes) for _, codes in CASES)
