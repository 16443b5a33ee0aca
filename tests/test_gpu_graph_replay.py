"""include/mvn.h promises calls that "never allocate, free or synchronise, so they can be graph-captured".  Here every launch path
of graph_replay_cases.py is held to it: one linear graph on one stream (torch.cuda.graph), all buffers allocated before the
capture, one eager warm-up call of the same shape, then ROUNDS replays, each on new contents written in place into the static
inputs -- weights, priors and costs too, with a NaN / +inf that comes and goes -- and after each replay the referee: the C oracle
bit for bit, or the eager call on the same inputs bit for bit.  Status words are 0 and columns >= T stay untouched.  The raw ABI is
called through mvn._lib; no test loops replays in the hope of a race: the stale-flag check at the end makes the one race this file
knows of (a replayed dealt launch taking a hand-off of the replay before) deterministic with the tests' build of the library."""
import ctypes

import numpy as np
import pytest
import torch

import graph_replay_cases as gc
import meta_viterbinet_amd as mvn

pytestmark = pytest.mark.gpu
P = mvn._lib.ptr
POISON = 7.0  # what outputs hold before a replay: neither a decision nor a metric of these inputs

ids = lambda cases: [c["id"] for c in cases]  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    n_cu, name = ctypes.c_int(), ctypes.create_string_buffer(64)
    assert mvn._lib.load().mvn_device_info(ctypes.byref(n_cu), None, name, 64) == 0, f"not a gfx950 device: {name.value!r}"
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _put(t, a):
    """new contents IN PLACE (the graph holds t's address)"""
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).view(t.dtype).reshape(t.shape))


def _set_env(monkeypatch, case):
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)


def _name(fn, *args):
    buf = ctypes.create_string_buffer(128)
    assert fn(*args, buf, 128) == 0
    return buf.value.decode()


def _st(dev):
    return mvn._lib.current_stream(dev)  # (the capture stream while torch.cuda.graph is open)


def _status(ws):
    return int(ws[:4].view(torch.int32).item())


def capture_and_replay(fill, call, check, rounds=gc.ROUNDS):
    """fill(round) writes the round's inputs in place and poisons the outputs; call() issues the ABI calls on the current stream;
    check(round) compares with the referee after the replay.  Returns the graph."""
    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # eager warm-up outside the capture: library load, dynamic-LDS attributes
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for rnd in range(1, rounds + 1):
        fill(rnd)
        graph.replay()
        torch.cuda.synchronize()
        check(rnd)
    return graph


def _eq(t, ref, what, nan=False):
    assert np.array_equal(_np(t), ref, equal_nan=nan), what


class Vnet:
    """The static buffers of one mvn_vnet_decode_f32 / mvn_vnet_decode_count_f32 capture."""

    def __init__(self, lib, dev, case, variant, zero_ws=False):
        self.lib, self.dev, self.case, self.variant = lib, dev, case, variant
        S, B, T = case.get("S", 16), case["B"], case["T"]
        self.S, self.B, self.T, self.ld = S, B, T, T + gc.PAD
        inp = gc.vnet_inputs(case, 0)
        self.y = torch.zeros(B, self.ld, device=dev)
        self.w = [torch.tensor(a, device=dev) for a in inp["w"]]
        self.dec = torch.empty(B, self.ld, device=dev)
        self.lg = torch.empty(B, T, S, device=dev) if variant == "logits" else None
        self.fm = torch.empty(B, S, device=dev) if variant != "count" else None
        self.K = inp["K"]
        self.tx = torch.zeros(B, self.K, device=dev)
        self.mask = torch.tensor(inp["mask"], device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.nb = int(lib.mvn_vnet_workspace_bytes(B, T, S))
        self.ws = torch.full((max(self.nb, 128),), 0 if zero_ws else 0x5A, dtype=torch.uint8, device=dev)
        self.expected = np.zeros(4, np.int64)

    def fill(self, rnd):
        inp = gc.vnet_inputs(self.case, rnd)
        _put(self.y, inp["y"])
        _put(self.tx, inp["tx"])
        for t, a in zip(self.w, inp["w"]):
            _put(t, a)
        for t in (self.dec, self.lg, self.fm):
            if t is not None:
                t.fill_(POISON)
        if rnd <= 1:
            self.counters.zero_()  # (the warm-up counted round 0; the replays accumulate from zero)

    def call(self):
        w = [P(t) for t in self.w]
        if self.variant == "count":
            rc = self.lib.mvn_vnet_decode_count_f32(P(self.y), self.ld, *w, P(self.tx), self.K, self.K, P(self.mask), P(self.counters),
                                                    P(self.dec), self.ld, P(self.ws), self.nb, self.B, self.T, self.S, _st(self.dev))
        else:
            rc = self.lib.mvn_vnet_decode_f32(P(self.y), self.ld, *w, P(self.dec), self.ld, P(self.lg), P(self.fm), P(self.ws), self.nb,
                                              self.B, self.T, self.S, _st(self.dev))
        assert rc == 0

    def check(self, rnd):
        ref, T = gc.vnet_referee(self.case, rnd), self.T
        _eq(self.dec[:, :T], ref["dec"], (rnd, "decisions"))
        assert bool((self.dec[:, T:] == POISON).all()), (rnd, "columns >= T were written")
        if self.fm is not None:
            _eq(self.fm, ref["final"], (rnd, "final metrics"), nan=True)
        if self.lg is not None:
            _eq(self.lg, ref["logits"], (rnd, "logits"), nan=True)
        if self.variant == "count":
            self.expected = self.expected + ref["counts"]
            assert self.counters.tolist() == self.expected.tolist(), (rnd, "the counters accumulate exactly")
        if "ring" in self.case:
            assert _status(self.ws) == 0, (rnd, "status word")


# ---- 1. ViterbiNet at 16 states ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", gc.VNET16_VARIANTS)
@pytest.mark.parametrize("case", gc.VNET16, ids=ids(gc.VNET16))
def test_vnet16_replays(oracle, dev, monkeypatch, case, variant):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    name = _name(lib.mvn_vnet_decode_kernel_name, case["B"], case["T"], 16, int(variant == "logits"))
    assert name.startswith(case["kernel"]) and ("ring" not in case or name.endswith(f"rings of {case['ring']}")), name
    v = Vnet(lib, dev, case, variant)
    assert "ring" not in case or v.nb == (min(case["B"], gc.DEALT_GROUPS) * (8 // case["ring"]) + 1) * 128
    capture_and_replay(v.fill, v.call, v.check)


# ---- 2. ViterbiNet at 4, 64 and 256 states: a weight of the last layer goes finite -> inf -> finite in place --------------------------
@pytest.mark.parametrize("case", gc.VNET_STATES, ids=ids(gc.VNET_STATES))
def test_vnet_states_replays_with_a_guard_launch_that_must_not_stick(oracle, dev, monkeypatch, case):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    assert _name(lib.mvn_vnet_decode_kernel_name, case["B"], case["T"], case["S"], 0).startswith(case["kernel"])
    v = Vnet(lib, dev, case, "plain")
    assert (v.nb == 0) == (case["route"] == "fused_ip")
    capture_and_replay(v.fill, v.call, v.check)


# ---- 3. classical Viterbi ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.VA, ids=ids(gc.VA))
def test_va_replays_with_a_nan_prior_that_comes_and_goes(oracle, dev, monkeypatch, case):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    S, B, T, Bp, ld = case["S"], case["B"], case["T"], case["Bp"], case["T"] + gc.PAD
    assert _name(lib.mvn_va_decode_kernel_name, B, T, S).startswith(case["kernel"])
    y, pri = torch.zeros(B, ld, device=dev), torch.zeros(Bp, S, device=dev)
    dec, fm = torch.empty(B, ld, device=dev), torch.empty(B, S, device=dev)

    def fill(rnd):
        inp = gc.va_inputs(case, rnd)
        _put(y, inp["y"])
        _put(pri, inp["pri"])
        dec.fill_(POISON)
        fm.fill_(POISON)

    def call():
        assert lib.mvn_va_decode_f32(P(y), ld, P(pri), Bp, P(dec), ld, P(fm), B, T, S, _st(dev)) == 0

    def check(rnd):
        ref = gc.va_referee(case, rnd)
        _eq(dec[:, :T], ref["dec"], (rnd, "decisions"))
        _eq(fm, ref["final"], (rnd, "final metrics"), nan=True)
        assert bool((dec[:, T:] == POISON).all()), (rnd, "columns >= T were written")

    capture_and_replay(fill, call, check)


@pytest.mark.parametrize("case", gc.SWEEP, ids=ids(gc.SWEEP))
def test_acs_sweep_replays_on_costs_that_gain_and_lose_a_nan(oracle, dev, monkeypatch, case):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    S, B, T, ld = case["S"], case["B"], case["T"], gc.sweep_ld(case["T"])
    cost = torch.zeros(B, T, S, device=dev)
    dec, fm = torch.empty(B, ld, device=dev), torch.empty(B, S, device=dev)
    assert _name(lib.mvn_acs_sweep_kernel_name, P(cost), P(dec), ld, B, T, S).startswith(case["kernel"])

    def fill(rnd):
        _put(cost, gc.sweep_inputs(case, rnd))
        dec.fill_(POISON)
        fm.fill_(POISON)

    def call():
        assert lib.mvn_acs_sweep_f32(P(cost), P(dec), ld, P(fm), B, T, S, _st(dev)) == 0

    def check(rnd):
        ref = gc.sweep_referee(gc.sweep_inputs(case, rnd))
        _eq(dec[:, :T], ref["dec"], (rnd, "decisions"))
        _eq(fm, ref["final"], (rnd, "final metrics"), nan=True)
        assert bool((dec[:, T:] == POISON).all()), (rnd, "columns >= T were written")

    capture_and_replay(fill, call, check)


def _surv_buffers(dev, B, T, S, ld):
    return dict(dec=torch.empty(B, ld, device=dev), fm=torch.empty(B, S, device=dev),
                surv=torch.empty(B, T, max(1, S // 8), dtype=torch.uint8, device=dev), bits=torch.empty(B, ld, device=dev),
                states=torch.empty(B, T, dtype=torch.int32, device=dev))


def _surv_poison(o):
    for k in ("dec", "fm", "bits"):
        o[k].fill_(POISON)
    o["surv"].fill_(0xA5)
    o["states"].fill_(-7)


def _surv_check(o, ref, T, rnd):
    _eq(o["dec"][:, :T], ref["dec"], (rnd, "decisions"))
    _eq(o["fm"], ref["final"], (rnd, "final metrics"), nan=True)
    _eq(o["surv"], ref["surv"], (rnd, "survivors"))
    _eq(o["bits"][:, :T], ref["bits"], (rnd, "traced-back bits"))
    _eq(o["states"], ref["states"], (rnd, "traced-back states"))
    assert bool((o["dec"][:, T:] == POISON).all()) and bool((o["bits"][:, T:] == POISON).all()), (rnd, "columns >= T were written")


@pytest.mark.parametrize("case", gc.SURV, ids=ids(gc.SURV))
def test_survivor_sweep_and_traceback_replay(oracle, dev, case):
    lib = mvn._lib.load()
    S, B, T, ld = case["S"], case["B"], case["T"], gc.sweep_ld(case["T"])
    cost, o = torch.zeros(B, T, S, device=dev), _surv_buffers(dev, B, T, S, ld)

    def fill(rnd):
        _put(cost, gc.sweep_inputs(case, rnd))
        _surv_poison(o)

    def call():
        assert lib.mvn_acs_sweep_surv_f32(P(cost), P(o["dec"]), ld, P(o["fm"]), P(o["surv"]), B, T, S, _st(dev)) == 0
        assert lib.mvn_traceback_f32(P(o["surv"]), P(o["fm"]), P(o["bits"]), ld, P(o["states"]), B, T, S, _st(dev)) == 0

    capture_and_replay(fill, call, lambda rnd: _surv_check(o, gc.surv_referee(gc.sweep_inputs(case, rnd)), T, rnd))


def test_vnet_dealt_survivor_form_replays(oracle, dev):
    """mvn_vnet_decode_surv_f32 at 1300 x 72: vnet16_dealt_kernel<false, true>, hand-off lines in the workspace."""
    case = gc.VNET_SURV[0]
    lib = mvn._lib.load()
    S, B, T, ld = 16, case["B"], case["T"], case["T"] + gc.PAD
    nb = int(lib.mvn_vnet_surv_workspace_bytes(B, T, S))
    assert nb % 128 == 0 and nb <= (8 * gc.DEALT_GROUPS + 1) * 128  # hand-off lines, not the batch's logits: the fused detector serves the call
    inp = gc.vnet_inputs(case, 0)
    y, w = torch.zeros(B, ld, device=dev), [torch.tensor(a, device=dev) for a in inp["w"]]
    ws, o = torch.full((nb,), 0x5A, dtype=torch.uint8, device=dev), _surv_buffers(dev, B, T, S, ld)

    def fill(rnd):
        _put(y, gc.vnet_inputs(case, rnd)["y"])
        _surv_poison(o)

    def call():
        assert lib.mvn_vnet_decode_surv_f32(P(y), ld, *[P(t) for t in w], P(o["dec"]), ld, P(o["fm"]), P(o["surv"]), P(ws), nb, B, T, S,
                                            _st(dev)) == 0
        assert lib.mvn_traceback_f32(P(o["surv"]), P(o["fm"]), P(o["bits"]), ld, P(o["states"]), B, T, S, _st(dev)) == 0

    def check(rnd):
        _surv_check(o, gc.vnet_surv_referee(case, rnd), T, rnd)
        assert _status(ws) == 0

    capture_and_replay(fill, call, check)


# ---- 4. codec and counting: encode -> corrupt in place -> decode with status -> count, one graph -----------------------------------
@pytest.mark.parametrize("case", gc.CODEC, ids=ids(gc.CODEC))
def test_codec_and_count_errors_replay(oracle, dev, case):
    lib = mvn._lib.load()
    nsym, n, B = case["nsym"], case["n"], case["B"]
    kb, nbits = 8 * (n - nsym), 8 * n
    ldo = kb + 4
    msg, flip, cw = torch.zeros(B, kb, device=dev), torch.zeros(B, nbits, device=dev), torch.empty(B, nbits, device=dev)
    out, status = torch.empty(B, ldo, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    counters, expected = torch.zeros(4, dtype=torch.int64, device=dev), [np.zeros(4, np.int64)]

    def fill(rnd):
        inp = gc.codec_inputs(case, rnd)
        _put(msg, inp["msg"])
        _put(flip, inp["flip"])
        cw.fill_(POISON)
        out.fill_(POISON)
        status.fill_(-7)
        if rnd <= 1:
            counters.zero_()

    def call():
        assert lib.mvn_rs_encode_bits_f32(P(msg), kb, P(cw), nbits, B, kb, nsym, _st(dev)) == 0
        cw.sub_(flip).abs_()  # |c - f| = c xor f on {0, 1}: the corruption, in place and inside the graph
        assert lib.mvn_rs_decode_bits_f32(P(cw), nbits, P(out), ldo, P(status), B, nbits, nsym, _st(dev)) == 0
        assert lib.mvn_count_errors(P(out), ldo, P(msg), kb, None, B, kb, P(counters), _st(dev)) == 0

    def check(rnd):
        ref = gc.codec_referee(case, rnd)
        _eq(cw, ref["word"], (rnd, "the corrupted codeword"))
        _eq(out[:, :kb], ref["msg"], (rnd, "decoded message"))
        _eq(status, ref["status"], (rnd, "decoder status"))
        assert bool((out[:, kb:] == POISON).all()), (rnd, "columns >= K were written")
        expected[0] = expected[0] + ref["counts"]
        assert counters.tolist() == expected[0].tolist(), (rnd, "the counters accumulate exactly")

    capture_and_replay(fill, call, check)


# ---- the stale-flag check --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.STALE, ids=ids(gc.STALE))
def test_replayed_dealt_launch_takes_no_handoff_of_an_earlier_replay(oracle, dev, case):
    """A captured dealt launch replays with the flag value ("nonce") it was captured with, and nothing in the kernel clears a flag:
    without help a ring that reaches its wait before this replay's producer has published finds the PREVIOUS replay's flag set
    and sweeps on from that replay's path metrics -- finite {0, 1} decisions, status 0, wrong.  The race is almost always won,
    so it is staged: the tests' build silences ring skip_ring's publication (captured with the launch; its consumer's wait is
    bounded by spin_limit polls), replay 1 shows the abandoned hand-off (status 1, one NaN tail) and which flag value the graph
    carries, then the silenced line is made to look as a previous replay would have left it -- POISON_METRICS, abandoned = 0,
    that flag value -- and replay 2 runs on new inputs.  Allowed: status 1, that block's tail NaN, everything else the oracle's
    (the launch cleared or ignored the line and waited in vain); or status 0 and every row the oracle's (captured launches kept
    off the hand-off).  Not allowed: status 0 with finite decisions that are not the oracle's.
    On the library of the commit before the fix (a captured launch without the memset node) replay 2 fails with
        rings8-1000x200: status 0 but block 7 continues from the previous replay's metrics: 2 of its decisions from symbol 160 on differ
        ring1-7000x100:  status 0 but block 10 continues from the previous replay's metrics: 3 of its decisions from symbol 32 on differ
    (the poisoned metrics decide the next four symbols 0 and merge with the oracle's path soon after: test_graph_replay_host.py)"""
    import __graft_entry__ as ge

    lib = mvn._lib.load_variant(ge.build_hip_hooks())
    lib.mvn_test_hooks_dealt.restype, lib.mvn_test_hooks_dealt.argtypes = None, [ctypes.c_int32, ctypes.c_int64]
    lib.mvn_reload_switches()
    B, T, skip = case["B"], case["T"], case["skip_ring"]
    assert _name(lib.mvn_vnet_decode_kernel_name, B, T, 16, 0) == f"vnet16_dealt_kernel<false> rings of {case['ring']}"
    v = Vnet(lib, dev, case, "plain", zero_ws=True)  # a caller-owned, zeroed workspace
    blk, t0 = gc.stale_block(case)
    v.fill(0)
    v.call()  # eager warm-up, nothing silenced
    torch.cuda.synchronize()
    v.check(0)
    try:
        lib.mvn_test_hooks_dealt(skip, case["spin_limit"])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            v.call()
    finally:
        lib.mvn_test_hooks_dealt(-1, 1 << 21)
    others = torch.ones(B, dtype=torch.bool, device=dev)
    others[blk] = False

    def abandoned(rnd):
        ref = gc.vnet_referee(case, rnd)["dec"]
        assert _status(v.ws) == 1, rnd
        assert bool(torch.isnan(v.dec[blk, t0:T]).all()) and np.array_equal(_np(v.dec[blk, :t0]), ref[blk, :t0]), rnd
        assert np.array_equal(_np(v.dec[others, :T]), ref[_np(others)]), rnd  # exactly one block with a NaN tail

    v.fill(1)
    graph.replay()
    torch.cuda.synchronize()
    abandoned(1)
    lines = v.ws.view(torch.int64).view(-1, 16)  # 128-byte lines: u64 9 is the flag of the metrics
    flag = int(lines[1 + gc.publishing_ring(case), 9].item())
    assert flag != 0 and int(lines[1 + skip, 9].item()) != flag  # a ring that published holds the graph's value, the silenced line does not
    line = v.ws[(1 + skip) * 128:(2 + skip) * 128]
    line.view(torch.float32)[:16] = torch.tensor(gc.POISON_METRICS, device=dev)
    line.view(torch.int32)[16] = 0
    line.view(torch.int64)[9] = flag
    v.fill(2)
    graph.replay()
    torch.cuda.synchronize()
    ref = gc.vnet_referee(case, 2)["dec"]
    if _status(v.ws) == 1:
        abandoned(2)
    else:
        got = _np(v.dec[blk, :T])
        assert np.array_equal(got, ref[blk], equal_nan=True), \
            f"status 0 but block {blk} continues from the previous replay's metrics: {int((got != ref[blk]).sum())} of its decisions from symbol {t0} on differ"
        assert np.array_equal(_np(v.dec[:, :T]), ref)


# ======================= 5 ... 8: the referee is the eager call on the same inputs, bit for bit ====================================
def _bits(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def replay_vs_eager(fill, call, outs, differ):
    """capture_and_replay, then the same rounds as eager calls on the same buffers: every output of every round bit for bit the
    replay's, and -- so that a replay on stale inputs could not pass -- outs[differ] of successive rounds (round 0, the captured
    content, included) differing in at least a tenth of their rows."""
    got = {}
    capture_and_replay(fill, call, lambda rnd: got.__setitem__(rnd, [t.clone() for t in outs]))
    prev = None
    for rnd in range(0, gc.ROUNDS + 1):
        fill(rnd)
        call()
        torch.cuda.synchronize()
        if rnd:
            for i, (g, t) in enumerate(zip(got[rnd], outs)):
                assert _same_bits(g, t), (rnd, i)
            assert gc.rows_that_differ(_np(outs[differ]), prev) >= 0.1, rnd
        prev = _np(outs[differ]).copy()


# ---- 5. LSTM: the pack kernel runs on every replay -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.LSTM, ids=ids(gc.LSTM))
def test_lstm_decode_replays_on_rewritten_weights(dev, case):
    lib = mvn._lib.load()
    B, T, ld = case["B"], case["T"], case["T"] + gc.PAD
    assert _name(lib.mvn_lstm_decode_kernel_name, B, T).startswith(case["kernel"])
    inp = gc.lstm_inputs(case, 0)
    y, w = torch.zeros(B, ld, device=dev), [torch.tensor(a, device=dev) for a in inp["w"]]
    dec, lg = torch.empty(B, ld, device=dev), torch.empty(B, T, 2, device=dev)
    nb = int(lib.mvn_lstm_workspace_bytes(B, T))
    ws = torch.full((max(nb, 16),), 0x5A, dtype=torch.uint8, device=dev)

    def fill(rnd):
        inp = gc.lstm_inputs(case, rnd)
        _put(y, inp["y"])
        for t, a in zip(w, inp["w"]):
            _put(t, a)
        dec.fill_(POISON)
        lg.fill_(POISON)

    def call():
        assert lib.mvn_lstm_decode_f32(P(y), ld, *[P(t) for t in w], P(dec), ld, P(lg), P(ws), nb, B, T, _st(dev)) == 0

    replay_vs_eager(fill, call, [dec, lg], differ=1)
    assert bool((dec[:, T:] == POISON).all()) and bool(((dec[:, :T] == 0) | (dec[:, :T] == 1)).all())


# ---- 6. the by-word block steps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.STEPS, ids=ids(gc.STEPS))
def test_byword_steps_replay(dev, case):
    import codec_cases

    lib = mvn._lib.load()
    R, K, nsym, S = gc.STEP_R, gc.STEP_K, gc.STEP_NSYM, case["S"]
    T = K + 8 * nsym
    if case["kind"] == "vnet":
        assert T <= int(lib.mvn_vnet_byword_step_max_symbols(S))
        g7 = np.load(codec_cases.__file__.replace("codec_cases.py", "golden/g7_by_word.npz"))
        w = [g7[f"w{i}"] for i in range(6)] if S == 16 else gc.rand_weights(S, np.random.RandomState(case["seed"]), scale=2.0)
        keep = [torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev) for a in w]
        front = (*[P(t) for t in keep], None)
    else:
        keep = torch.tensor(codec_cases.channel()[1], device=dev)
        front = (P(keep), 1)
    ld = T + gc.PAD
    rx, tx = torch.zeros(R, ld, device=dev), torch.zeros(R, K + gc.PAD, device=dev)
    f32 = {n: torch.empty(R, (K if n == "msg" else T) + gc.PAD, device=dev) for n in ("dec", "msg", "enc", "lw", "delta")}
    labels, nerr = torch.empty(R, ld, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    choice = torch.empty(R, dtype=torch.int32, device=dev)
    tail = (case["list_bytes"], P(f32["delta"]), ld, P(choice)) if "list_bytes" in case else ()

    def fill(rnd):
        inp = gc.step_inputs(case, rnd)
        rx[:, :T].copy_(torch.from_numpy(inp["rx"]))
        tx[:, :K].copy_(torch.from_numpy(inp["tx"]))
        for t in f32.values():
            t.fill_(POISON)
        for t in (labels, nerr, choice):
            t.fill_(-7)

    def call():
        rc = getattr(lib, case["fn"])(P(rx), ld, P(tx), K + gc.PAD, *front, P(f32["dec"]), ld, P(f32["msg"]), K + gc.PAD, P(f32["enc"]), ld,
                                      P(f32["lw"]), ld, P(labels), ld, P(nerr), R, T, nsym, 0, S, *tail, _st(dev))
        assert rc == 0

    outs = [f32["dec"], f32["msg"], f32["enc"], f32["lw"], labels, nerr] + ([f32["delta"], choice] if tail else [])
    replay_vs_eager(fill, call, outs, differ=2)
    for n, t in f32.items():
        if n != "delta" or tail:
            width = K if n == "msg" else T
            assert bool((t[:, width:] == POISON).all()) and not bool((t[:, :width] == POISON).any()), n
    assert bool((labels[:, T:] == -7).all()) and bool((nerr >= 0).all())


# ---- 7. training: n replays = n eager calls, weights, moments and losses bit for bit -------------------------------------------------
def train_replay_vs_eager(state, fill, call, loss, status):
    """`state`: the tensors a call updates in place.  Warm-up, capture, ROUNDS replays (a new word each), then from the same start
    ROUNDS eager calls on the same words."""
    start = [t.clone() for t in state]

    def restore():
        for t, s in zip(state, start):
            t.copy_(s)

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    losses = []
    for rnd in range(1, gc.ROUNDS + 1):
        fill(rnd)
        loss.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert int(status.abs().max().item()) == 0, rnd
        assert bool(torch.isfinite(loss).all()) and not bool((loss == POISON).any()), rnd
        losses.append(loss.clone())
    assert not torch.equal(losses[0], losses[1]) and not torch.equal(losses[1], losses[2])
    replayed = [t.clone() for t in state]
    assert not _same_bits(replayed[0], start[0])  # the weights moved
    restore()
    for rnd in range(1, gc.ROUNDS + 1):
        fill(rnd)
        loss.fill_(POISON)
        call()
        torch.cuda.synchronize()
        assert _same_bits(loss, losses[rnd - 1]), (rnd, "losses")
    for i, (a, t) in enumerate(zip(replayed, state)):
        assert _same_bits(a, t), ("state tensor", i)


@pytest.mark.parametrize("case", gc.TRAIN, ids=ids(gc.TRAIN))
def test_online_training_replays(dev, monkeypatch, case):
    _set_env(monkeypatch, case)
    lib = mvn._lib.load()
    S, T, n_iter = case["S"], gc.TRAIN_T, gc.TRAIN_ITERS
    M = 0 if case["whole_word"] else gc.TRAIN_M
    nb = int(lib.mvn_vnet_train_workspace_bytes(S))
    assert _name(lib.mvn_vnet_train_kernel_name, 0, 0, T, M, S, nb).startswith(case["kernel"])
    w = [torch.tensor(a, device=dev) for a in gc.rand_weights(S, np.random.RandomState(case["seed"]))]
    n = sum(t.numel() for t in w)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    y, labels = torch.zeros(T, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)
    idx = torch.zeros(n_iter, gc.TRAIN_M, dtype=torch.int32, device=dev)
    loss, status = torch.empty(n_iter, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.full((max(nb, 16),), 0x5A, dtype=torch.uint8, device=dev)
    b1, b2, eps = {"Adam": gc.ADAM, "RMSprop": gc.RMSPROP, "SGD": gc.SGD}[case["opt"]]
    lr = 0.05 if case["opt"] == "SGD" else 1e-3

    def fill(rnd):
        inp = gc.train_inputs(case, rnd)
        _put(y, inp["y"])
        _put(labels, inp["labels"])
        _put(idx, inp["idx"])

    def call():
        rc = lib.mvn_vnet_online_train_ws_f32(P(y), P(labels), T, P(idx) if M else None, M, n_iter, *[P(t) for t in w], P(m), P(v),
                                              case["step0"], lr, b1, b2, eps, P(loss), S, P(ws), nb, P(status), _st(dev))
        assert rc == 0

    train_replay_vs_eager(w + [m, v], fill, call, loss, status)


def test_online_training_trials_replay_with_adam_powers_rewritten_in_the_descriptors(dev):
    """mvn_vnet_online_train_trials_f32, Adam, two trials: the step count reaches the kernel as beta1^t / beta2^t in the DEVICE
    descriptors, which the caller rewrites in place between replays -- so a replayed Adam step is the eager one."""
    from meta_viterbinet_amd import trials as tr_mod

    lib = mvn._lib.load()
    case = dict(S=16, seed=4242)
    R, S, T, M, n_iter = 2, 16, gc.TRAIN_T, gc.TRAIN_M, gc.TRAIN_ITERS
    assert _name(lib.mvn_vnet_train_kernel_name, 0, R, T, M, S, 0) == f"online_train_kernel<{S}, true> 1x{R}"
    rng = np.random.RandomState(77)
    bank = tr_mod.TrialBank([gc.rand_weights(S, rng) for _ in range(R)], S, 4, dev, lr=1e-3, optimizer_type="Adam")
    y, labels = torch.zeros(R, T, device=dev), torch.zeros(R, T, dtype=torch.int32, device=dev)
    idx = torch.zeros(R, n_iter, M, dtype=torch.int32, device=dev)
    loss, status = torch.empty(R, n_iter, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    d = np.zeros(R, dtype=tr_mod.TRIAL_DTYPE)
    dd = torch.zeros(d.nbytes, dtype=torch.uint8, device=dev)
    th = bank.pointers(bank.theta)
    for r in range(R):
        d[r]["y"], d[r]["labels"], d[r]["idx"] = y[r].data_ptr(), labels[r].data_ptr(), idx[r].data_ptr()
        d[r]["w_in"], d[r]["w_out"] = th[r], th[r]
        d[r]["adam_m"], d[r]["adam_v"] = bank.exp_avg[r].data_ptr(), bank.exp_avg_sq[r].data_ptr()
        d[r]["loss_out"], d[r]["status"] = loss[r].data_ptr(), status[r:].data_ptr()
        d[r]["n"] = n_iter

    def fill(rnd):
        for r in range(R):
            inp = gc.train_inputs(dict(case, seed=case["seed"] + r), rnd)
            _put(y[r], inp["y"])
            _put(labels[r], inp["labels"])
            _put(idx[r], inp["idx"])
            steps = n_iter * max(rnd - 1, 0)  # Adam steps taken before this round's call
            d[r]["b1pow"], d[r]["b2pow"] = 0.9 ** steps, 0.999 ** steps
        dd.copy_(torch.from_numpy(d.view(np.uint8).copy()))

    def call():
        assert lib.mvn_vnet_online_train_trials_f32(P(dd), R, T, M, 1e-3, *gc.ADAM, S, None, 0, _st(dev)) == 0

    train_replay_vs_eager([bank.theta, bank.exp_avg, bank.exp_avg_sq], fill, call, loss, status)
    assert not torch.equal(bank.theta[0], bank.theta[1])


def test_lstm_training_replays(dev):
    """mvn_lstm_train_f32 with SGD at T = 5 (a hipMemsetAsync of its GroupSync in front of the kernel)."""
    lib = mvn._lib.load()
    case = dict(gc.LSTM[0], B=1)
    T, n_iter = 5, 2
    assert _name(lib.mvn_lstm_train_kernel_name, T, 0).startswith("lstm_train_kernel x ")
    w = [torch.tensor(a, device=dev) for a in gc.lstm_inputs(case, 0)["w"]]
    n = sum(t.numel() for t in w)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    y, bits = torch.zeros(1, T, device=dev), torch.zeros(1, T, dtype=torch.int32, device=dev)
    loss, status = torch.empty(n_iter, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    nb = int(lib.mvn_lstm_train_workspace_bytes(T))
    ws = torch.full((max(nb, 16),), 0x5A, dtype=torch.uint8, device=dev)

    def fill(rnd):
        rng = np.random.RandomState(900 + rnd)
        _put(y, rng.normal(0, 1.5, (1, T)).astype(np.float32))
        _put(bits, rng.randint(0, 2, (1, T)).astype(np.int32))

    def call():
        rc = lib.mvn_lstm_train_f32(P(y), T, P(bits), T, 1, None, None, 0, n_iter, *[P(t) for t in w], P(m), P(v), 0, 0.05, *gc.SGD, P(loss),
                                    P(ws), nb, P(status), T, _st(dev))
        assert rc == 0

    train_replay_vs_eager(w + [m, v], fill, call, loss, status)


# ---- 8. Monte-Carlo: seed and word0 are frozen, so two replays count exactly twice what one eager call counts ----------------------
CC = {"train": "time_decay", "val": "time_decay"}


def _twice_the_eager_counters(call, counters, extra=()):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = counters.tolist()
    eager_extra = [t.clone() for t in extra]
    assert eager[1] > 0 and eager[0] > 0 and eager[3] > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    counters.zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert counters.tolist() == [2 * c for c in eager]
    for a, t in zip(eager_extra, extra):
        assert torch.equal(a, t)


@pytest.mark.parametrize("case", gc.MONTECARLO, ids=ids(gc.MONTECARLO))
def test_va_montecarlo_replays(dev, case):
    lib = mvn._lib.load()
    S, L, B, T = case["S"], case["L"], case["B"], case["T"]
    h = np.ascontiguousarray(mvn.estimate_channel(L, 0.2, "time_decay"), dtype=np.float64).reshape(-1, L)
    va = mvn.VADetector(S, L, T, 1, "ISI_AWGN", 0, False, 1, CC)
    pri = torch.tensor(np.ascontiguousarray(_np(va.compute_state_priors(h)).T, dtype=np.float32), device=dev)
    assert tuple(pri.shape) == (1, S)
    hd, counters = torch.tensor(h, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    sigma = float((10 ** (2.0 / 10)) ** (-0.5))  # 2 dB: errors to count

    def call():
        assert lib.mvn_va_montecarlo_f32(P(hd), hd.shape[0], sigma, case["seed"], P(pri), 1, P(counters), B, T, L, S, _st(dev)) == 0

    _twice_the_eager_counters(call, counters)


def test_vnet_montecarlo_replays_with_rounds_and_a_stop_rule(dev):
    """mvn_vnet_montecarlo_f32 with n_rounds = 3 and a stop rule: `progress` is zeroed by a captured zero_() in front of the call.
    The rule reads the ACCUMULATED counters[2] (include/mvn.h), so two replays count twice the eager call only while it does not
    fire: first with a threshold out of reach (every gate kernel runs, all three rounds run, twice); then with one that stops the
    point after its first round, the caller zeroing the counters in place between the replays: every replay the eager call's
    integers and the eager call's `progress`."""
    import codec_cases

    lib = mvn._lib.load()
    B, T, L, S = 300, 136, 4, 16
    g7 = np.load(codec_cases.__file__.replace("codec_cases.py", "golden/g7_by_word.npz"))
    w = [torch.tensor(np.ascontiguousarray(g7[f"w{i}"], dtype=np.float32), device=dev) for i in range(6)]
    hd = torch.tensor(np.ascontiguousarray(mvn.estimate_channel(L, 0.2, "time_decay"), dtype=np.float64).reshape(-1, L), device=dev)
    counters, progress = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    sigma = float((10 ** (6.0 / 10)) ** (-0.5))

    def point(stop):
        def call():
            progress.zero_()
            assert lib.mvn_vnet_montecarlo_f32(P(hd), hd.shape[0], sigma, 20261, 7, *[P(t) for t in w], P(counters), P(progress), B, 3, stop,
                                               T, L, S, _st(dev)) == 0
        return call

    _twice_the_eager_counters(point(10 ** 6), counters, extra=[progress])
    assert int(progress[0].item()) == 3 and counters[3].item() == 2 * 3 * B and counters[2].item() >= 10
    counters.zero_()
    call = point(5)
    call()
    torch.cuda.synchronize()
    eager, eager_progress = counters.tolist(), progress.clone()
    assert int(eager_progress[0].item()) == 1 and eager[3] == B and eager[2] >= 5  # the rule fired after the first round
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        counters.zero_()
        progress.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert counters.tolist() == eager and torch.equal(progress, eager_progress)
