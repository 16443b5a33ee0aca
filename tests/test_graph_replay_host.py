"""Does the table of graph_replay_cases.py bite?  CPU only: the library's kernel-name queries (they answer without a device,
assuming 256 CUs) and the C oracle.  A case that names another kernel than it intends, a dealt case without a hand-off through
the workspace, replays whose referee outputs hardly differ, or an in-place NaN / inf that changes nothing would let the GPU
tests of test_gpu_graph_replay.py pass on a library that replays wrongly."""
import ctypes

import numpy as np
import pytest

import graph_replay_cases as gc
import meta_viterbinet_amd as mvn

ids = lambda cases: [c["id"] for c in cases]  # noqa: E731


def _set_env(monkeypatch, case):
    for k in ("MVN_COOP", "MVN_DEALT", "MVN_UNFUSED", "MVN_FUSED_IP", "MVN_FUSEDN", "MVN_VA16", "MVN_VA_INPLACE", "MVN_VA256",
              "MVN_GENERIC_SWEEP", "MVN_SWEEP_INPLACE", "MVN_SWEEP16"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    mvn._lib.load().mvn_reload_switches()


def _name(fn, *args):
    buf = ctypes.create_string_buffer(128)
    assert fn(*args, buf, 128) == 0
    return buf.value.decode()


@pytest.mark.parametrize("case", gc.VNET16 + gc.STALE, ids=ids(gc.VNET16 + gc.STALE))
def test_vnet16_cases_name_their_kernels(monkeypatch, case):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    for want_logits in (0, 1):
        name = _name(lib.mvn_vnet_decode_kernel_name, case["B"], case["T"], 16, want_logits)
        assert name.startswith(case.get("kernel", "vnet16_dealt_kernel<")), name
        if "ring" in case:
            assert name.endswith(f"rings of {case['ring']}"), name
            assert int(lib.mvn_vnet_workspace_bytes(case["B"], case["T"], 16)) == (gc.DEALT_GROUPS * (8 // case["ring"]) + 1) * 128


@pytest.mark.parametrize("case", [c for c in gc.VNET16 + gc.STALE if "ring" in c], ids=lambda c: c["id"])
def test_dealt_cases_hand_blocks_across_rings(case):
    """Most rings end inside a block, so their last unit's metrics travel through a workspace line -- and the ring the
    stale-flag check silences is one of them, cutting its block neither at the block's start nor in its last unit."""
    n_rings = min(case["B"], gc.DEALT_GROUPS) * (8 // case["ring"])
    assert gc.dealt_crossings(case) >= n_rings // 2
    if "skip_ring" in case:
        b, t0 = gc.stale_block(case)
        assert 0 < t0 < case["T"] - 8 and 0 <= b < case["B"]


@pytest.mark.parametrize("case", gc.VNET_STATES, ids=ids(gc.VNET_STATES))
def test_vnet_states_cases_name_their_kernels(monkeypatch, case):
    _set_env(monkeypatch, case)
    name = _name(mvn._lib.load().mvn_vnet_decode_kernel_name, case["B"], case["T"], case["S"], 0)
    assert name.startswith(case["kernel"]), name


@pytest.mark.parametrize("case", gc.VA, ids=ids(gc.VA))
def test_va_cases_name_their_kernels(monkeypatch, case):
    _set_env(monkeypatch, case)
    name = _name(mvn._lib.load().mvn_va_decode_kernel_name, case["B"], case["T"], case["S"])
    assert name.startswith(case["kernel"]), name


@pytest.mark.parametrize("case", gc.SWEEP, ids=ids(gc.SWEEP))
def test_sweep_cases_name_their_kernels(monkeypatch, case):
    _set_env(monkeypatch, case)
    name = _name(mvn._lib.load().mvn_acs_sweep_kernel_name, None, None, gc.sweep_ld(case["T"]), case["B"], case["T"], case["S"])
    assert name.startswith(case["kernel"]), name


def _assert_rounds_differ(outputs):
    """outputs: per round 1 ... ROUNDS (and 0, the captured content) a dict of referee arrays with one row per block"""
    for rnd in range(1, gc.ROUNDS + 1):
        for key in ("dec", "bits", "msg"):
            if key in outputs[rnd]:
                assert gc.rows_that_differ(outputs[rnd][key], outputs[rnd - 1][key]) >= 0.1, (rnd, key)


@pytest.mark.parametrize("case", gc.VNET16 + gc.VNET_STATES + gc.VNET_SURV + gc.STALE,
                         ids=ids(gc.VNET16 + gc.VNET_STATES + gc.VNET_SURV + gc.STALE))
def test_vnet_referee_changes_from_replay_to_replay(oracle, case):
    refs = [gc.vnet_referee(case, rnd) for rnd in range(gc.ROUNDS + 1)]
    _assert_rounds_differ(refs)
    if case in gc.VNET16:  # (the counting call: a replay that counted the previous round's words again adds another number)
        assert all(refs[rnd]["counts"][0] != refs[rnd - 1]["counts"][0] for rnd in range(1, gc.ROUNDS + 1))
    if case in gc.VNET_STATES:  # the +inf of the odd round changes what the oracle decides: a guard that never fired would fail
        inp = gc.vnet_inputs(case, gc.ODD_ROUND)
        assert not np.isfinite(inp["w"][4]).all() and all(np.isfinite(gc.vnet_inputs(case, r)["w"][4]).all() for r in (0, 1, 3))
        twin = oracle.vnet_decode(np.ascontiguousarray(inp["y"][:, :case["T"]]), gc.finite_twin(inp["w"]))
        assert gc.rows_that_differ(refs[gc.ODD_ROUND]["dec"], twin) >= 0.1


@pytest.mark.parametrize("case", gc.VA, ids=ids(gc.VA))
def test_va_referee_changes_and_the_nan_prior_matters(oracle, case):
    refs = [gc.va_referee(case, rnd) for rnd in range(gc.ROUNDS + 1)]
    _assert_rounds_differ(refs)
    pri = gc.va_inputs(case, gc.ODD_ROUND)["pri"]
    assert np.isnan(pri).sum() == 1 and all(np.isfinite(gc.va_inputs(case, r)["pri"]).all() for r in (0, 1, 3))
    twin = gc.va_referee(case, gc.ODD_ROUND, gc.va_finite_twin(pri))
    # (with a table row per block the NaN reaches its own block only)
    changed = gc.rows_that_differ(refs[gc.ODD_ROUND]["dec"], twin["dec"])
    assert changed >= 0.1 if case["Bp"] == 1 else changed * case["B"] >= 1
    assert not np.array_equal(refs[gc.ODD_ROUND]["final"], twin["final"], equal_nan=True)


@pytest.mark.parametrize("case", gc.SWEEP + gc.SURV, ids=ids(gc.SWEEP + gc.SURV))
def test_sweep_referee_changes_and_the_nan_costs_matter(oracle, case):
    ref = gc.surv_referee if case in gc.SURV else gc.sweep_referee
    refs = [ref(gc.sweep_inputs(case, rnd)) for rnd in range(gc.ROUNDS + 1)]
    _assert_rounds_differ(refs)
    cost = gc.sweep_inputs(case, gc.ODD_ROUND)
    assert np.isnan(cost).any() and all(np.isfinite(gc.sweep_inputs(case, r)).all() for r in (0, 1, 3))
    twin = ref(gc.sweep_finite_twin(cost))
    assert gc.rows_that_differ(refs[gc.ODD_ROUND]["dec"], twin["dec"]) >= 0.1


def test_vnet_surv_referee_changes_from_replay_to_replay(oracle):
    case = gc.VNET_SURV[0]
    _assert_rounds_differ([gc.vnet_surv_referee(case, rnd) for rnd in range(gc.ROUNDS + 1)])


@pytest.mark.parametrize("case", gc.CODEC, ids=ids(gc.CODEC))
def test_codec_cases_cover_zero_to_t_plus_one_byte_errors(oracle, case):
    refs = [gc.codec_referee(case, rnd) for rnd in range(gc.ROUNDS + 1)]
    _assert_rounds_differ(refs)
    seen, statuses = set(), set()
    for rnd in range(1, gc.ROUNDS + 1):
        inp = gc.codec_inputs(case, rnd)
        seen |= set(inp["n_err"].tolist())
        statuses |= set(refs[rnd]["status"].tolist())
        assert refs[rnd]["counts"][0] > 0 and refs[rnd]["counts"][0] != refs[rnd - 1]["counts"][0]
        ok = inp["n_err"] <= inp["t"]  # up to t byte errors are corrected, t + 1 are not
        assert np.array_equal(refs[rnd]["msg"][ok], inp["msg"][ok]) and (refs[rnd]["msg"][~ok] != inp["msg"][~ok]).any()
    assert seen == set(range(case["nsym"] // 2 + 2))
    assert 0 in statuses and statuses <= {0, 1, 2}


@pytest.mark.parametrize("case", gc.STALE, ids=ids(gc.STALE))
def test_poison_metrics_change_the_blocks_continuation(oracle, case):
    """The stale-flag check writes POISON_METRICS where a previous replay's publication would stand: a ring that took them would
    continue its block with other decisions than the oracle's -- finite {0, 1} ones -- in every replay the check looks at."""
    b, t0 = gc.stale_block(case)
    T = case["T"]
    for rnd in range(1, gc.ROUNDS + 1):
        inp, ref = gc.vnet_inputs(case, rnd), gc.vnet_referee(case, rnd)
        y_row = np.ascontiguousarray(inp["y"][b, :T])
        if rnd == 1:  # continue_from is the oracle's recurrence: entered with the oracle's own metrics it gives the oracle's tail
            lg = ref["logits"][b]
            m = np.zeros(16, np.float32)
            for t in range(t0):
                m = oracle.acs_block(m[None, :], -lg[t][None, :])[0][0]
            assert np.array_equal(gc.continue_from(y_row, inp["w"], t0, m), ref["dec"][b, t0:])
        poisoned = gc.continue_from(y_row, inp["w"], t0, gc.POISON_METRICS)
        assert set(poisoned.tolist()) <= {0.0, 1.0} and not np.array_equal(poisoned, ref["dec"][b, t0:]), rnd


# ---- the cases whose referee is the eager call (no CPU twin of their outputs here): the route and the inputs ------------------------
@pytest.mark.parametrize("case", gc.LSTM, ids=ids(gc.LSTM))
def test_lstm_cases_name_their_kernels_and_rewrite_every_weight(case):
    assert _name(mvn._lib.load().mvn_lstm_decode_kernel_name, case["B"], case["T"]).startswith(case["kernel"])
    for rnd in range(1, gc.ROUNDS + 1):
        a, b = gc.lstm_inputs(case, rnd), gc.lstm_inputs(case, rnd - 1)
        assert all(not np.array_equal(x, y) for x, y in zip(a["w"], b["w"])) and gc.rows_that_differ(a["y"], b["y"]) == 1.0


@pytest.mark.parametrize("case", [c for c in gc.TRAIN if c["form"] != "chunked"], ids=lambda c: c["id"])
def test_training_cases_name_their_kernels(monkeypatch, case):
    """(the one-workgroup-per-chunk form is planned from the device's CUs: its name is asserted on the GPU)"""
    monkeypatch.setenv("MVN_TRAIN_GROUPS", case["env"]["MVN_TRAIN_GROUPS"])
    lib = mvn._lib.load()
    lib.mvn_reload_switches()
    nb = int(lib.mvn_vnet_train_workspace_bytes(case["S"]))
    assert _name(lib.mvn_vnet_train_kernel_name, 0, 0, gc.TRAIN_T, gc.TRAIN_M, case["S"], nb).startswith(case["kernel"])
    words = [gc.train_inputs(case, rnd) for rnd in range(gc.ROUNDS + 1)]
    assert all(not np.array_equal(words[r]["y"], words[r - 1]["y"]) and not np.array_equal(words[r]["idx"], words[r - 1]["idx"])
               and words[r]["labels"].max() >= case["S"] // 2 for r in range(1, gc.ROUNDS + 1))


@pytest.mark.parametrize("case", gc.STEPS, ids=ids(gc.STEPS))
def test_step_cases_take_other_words_every_round(oracle, case):
    lib = mvn._lib.load()
    T = gc.STEP_K + 8 * gc.STEP_NSYM
    limit = {"mvn_vnet_byword_step_f32": lib.mvn_vnet_byword_step_max_symbols, "mvn_va_byword_step_f32": lib.mvn_va_byword_step_max_symbols,
             "mvn_vnet_byword_step_states_f32": lib.mvn_vnet_byword_step_max_symbols,
             "mvn_va_byword_step_list_f32": lib.mvn_va_byword_step_list_max_symbols}[case["fn"]]
    assert T <= int(limit(case["S"]))
    rounds = [gc.step_inputs(case, rnd) for rnd in range(gc.ROUNDS + 1)]
    for rnd in range(1, gc.ROUNDS + 1):
        assert rounds[rnd]["rx"].shape == (gc.STEP_R, T) and rounds[rnd]["tx"].shape == (gc.STEP_R, gc.STEP_K)
        assert gc.rows_that_differ(rounds[rnd]["tx"], rounds[rnd - 1]["tx"]) == 1.0
