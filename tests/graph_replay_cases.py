"""The case table of the graph-replay tests: which launch paths are captured, at which shapes, under which MVN_* switches, what
each replay's inputs are and what the referee says about them.  CPU only (numpy + the C oracle); no tests of its own: imported by
test_graph_replay_host.py (does the table bite?) and test_gpu_graph_replay.py (the captures).

A case is a dict: id, the shape, env (the switches that pin its route), kernel (what the library's *_kernel_name query must
answer, as a prefix / substring).  Round 0 is the content of the warm-up call and of the capture; rounds 1 ... ROUNDS are the
replays, every one on new contents written in place.  Inputs are a pure function of (case, round), so the CPU checks and the GPU
tests see the same numbers, and referee() caches what the oracle made of them (shared by the variants of a case; never modified).

The in-place changes that must not stick: in round ODD_ROUND one weight of the last layer is +inf (ViterbiNet off 16 states: the
guard launch fires on that replay only), one state prior is NaN (classical Viterbi), some costs are NaN (sweeps); the rounds
before and after are finite.
"""
import functools

import numpy as np

import oracle

ROUNDS = 3
ODD_ROUND = 2
PAD = 3  # y and dec rows are T + PAD long: columns >= T must come back untouched


def sweep_ld(T):
    """Row stride of a sweep's decisions: past T, and a multiple of 4 (the LDS-DMA kernels store float4 decisions)."""
    return T + (-T) % 4 + 4


def rand_weights(S, rng, scale=1.0):
    return [(rng.uniform(-1, 1, (100, 1)) * scale).astype(np.float32), rng.uniform(-1, 1, 100).astype(np.float32),
            rng.uniform(-0.1, 0.1, (50, 100)).astype(np.float32), rng.uniform(-0.1, 0.1, 50).astype(np.float32),
            rng.uniform(-0.14, 0.14, (S, 50)).astype(np.float32), rng.uniform(-0.14, 0.14, S).astype(np.float32)]


def _rng(case, rnd, salt=0):
    return np.random.RandomState((case["seed"] * 31 + rnd * 1009 + salt) % (2 ** 31))


def _seeded(cases):
    for i, c in enumerate(cases):
        c["seed"] = 7001 + 97 * i + c.get("S", 16)
    return cases


# ---- 1. ViterbiNet at 16 states: mvn_vnet_decode_f32 (variants "plain", "logits") and mvn_vnet_decode_count_f32 ("count") --------
# (9 x 136 with MVN_DEALT=0 alone is the cooperative kernel's: MVN_COOP=0 sends it to the one-wave-per-block kernel)
VNET16 = _seeded([
    dict(id="coop-64x136", B=64, T=136, env={}, kernel="vnet16_coop_kernel<"),
    dict(id="dealt8-1000x200", B=1000, T=200, env={}, kernel="vnet16_dealt_kernel<", ring=8),
    dict(id="dealt4-3100x130", B=3100, T=130, env={"MVN_DEALT": "4"}, kernel="vnet16_dealt_kernel<", ring=4),
    dict(id="ring1-7000x100", B=7000, T=100, env={}, kernel="vnet16_dealt_kernel<", ring=1),
    dict(id="fusedn-9x136", B=9, T=136, env={"MVN_DEALT": "0", "MVN_COOP": "0"}, kernel="vnet16_fusedn_kernel<"),
    dict(id="unfused-5x33", B=5, T=33, env={"MVN_UNFUSED": "1"}, kernel="mlp_kernel<1> + "),
])
VNET16_VARIANTS = ("plain", "logits", "count")
DEALT_GROUPS = 768  # 3 workgroups per CU at 256 CUs (what the name queries assume without a device, and what an MI355X has)


def dealt_crossings(case, groups=DEALT_GROUPS):
    """How many rings of the dealt launch end inside a block (a hand-off through the workspace), by the kernel's own cut:
    ring g owns units [N g / n, N (g + 1) / n) of the B x ceil(T / 32) block-major units."""
    U = (case["T"] + 31) // 32
    n = min(case["B"], groups) * (8 // case["ring"])
    N = case["B"] * U
    return sum(1 for g in range(n - 1) if (N * (g + 1) // n) % U)


# ---- 2. ViterbiNet at 4, 64 and 256 states: the fused in-place kernel and the two-kernel route ------------------------------------
VNET_STATES = _seeded([
    dict(id=f"S{S}-{route}-{B}x{T}", S=S, B=B, T=T, route=route,
         env={"MVN_FUSED_IP": "1", "MVN_UNFUSED": "0" if route == "fused_ip" else "1"},
         kernel="vnet_fused_ip_kernel<" if route == "fused_ip" else "mlp_kernel<")
    for S in (4, 64, 256) for route in ("fused_ip", "two_kernel") for B, T in ((5, 17), (70, 136))])

# ---- 3. classical Viterbi --------------------------------------------------------------------------------------------------------
VA = _seeded([
    dict(id=f"S{S}-{tag}-{B}x{T}-Bp{'B' if per_block else 1}", S=S, B=B, T=T, Bp=B if per_block else 1, env=env, kernel=kernel)
    for S, tag, env, kernel in ((16, "tile", {"MVN_VA16": "tile"}, "va16_tile_kernel"), (16, "split", {"MVN_VA16": "split"}, "va16_split_kernel"),
                                (16, "quad", {"MVN_VA16": "quad"}, "va16_quad_kernel"), (4, "inplace", {}, "va_inplace_kernel<0>"),
                                (64, "inplace", {}, "va_inplace_kernel<4>"), (256, "wave", {}, "va256_wave_kernel"))
    for B, T in ((6, 40), (131, 257)) for per_block in (False, True)])
SWEEP = _seeded([dict(id=f"S{S}-{B}x{T}", S=S, B=B, T=T, env={}, kernel=kernel)
                 for S, kernel in ((16, "sweep16_"), (64, "sweep_inplace_kernel<4")) for B, T in ((35, 40), (67, 129))])
SURV = _seeded([dict(id=f"S{S}-35x40", S=S, B=35, T=40, env={}) for S in (16, 64)])
VNET_SURV = _seeded([dict(id="dealt-surv-1300x72", S=16, B=1300, T=72, env={})])

# ---- 4. codec and counting ---------------------------------------------------------------------------------------------------------
CODEC = _seeded([dict(id=f"nsym{nsym}-n{n}", nsym=nsym, n=n, B=129, env={}) for nsym, n in ((2, 17), (8, 128))])


# ---- 5 ... 8: the referee is the eager call on the same inputs (the oracle has no LSTM, no codec step, no trainer) --------------------
LSTM = _seeded([dict(id=f"{B}x{T}", B=B, T=T, env={}, kernel="lstm_pack_kernel + lstm_decode_kernel<") for B, T in ((17, 5), (33, 136))])
LSTM_SHAPES = [(1024, 4), (1024, 256), (1024,), (1024,), (1024, 256), (1024, 256), (1024,), (1024,), (2, 256), (2,)]
STEP_R, STEP_K, STEP_NSYM, STEP_LIST_BYTES = 5, 120, 2, 6
STEPS = _seeded([dict(id="vnet", fn="mvn_vnet_byword_step_f32", kind="vnet", S=16, env={}),
                 dict(id="va", fn="mvn_va_byword_step_f32", kind="va", S=16, env={}),
                 dict(id="vnet-states-64", fn="mvn_vnet_byword_step_states_f32", kind="vnet", S=64, env={}),
                 dict(id="va-list", fn="mvn_va_byword_step_list_f32", kind="va", S=16, list_bytes=STEP_LIST_BYTES, env={})])
TRAIN_T, TRAIN_M, TRAIN_ITERS = 136, 33, 3
ADAM, RMSPROP, SGD = (0.9, 0.999, 1e-8), (-1.0, 0.99, 1e-8), (-2.0, 0.0, 0.0)  # (beta1, beta2, eps) as the kernels take them
TRAIN = _seeded(
    [dict(id=f"S{S}-{form}-{opt}", S=S, form=form, opt=opt, step0=0, whole_word=form == "chunked",
          env={"MVN_TRAIN_GROUPS": "1" if form == "chunked" else "0"},
          kernel=f"online_train_groups_kernel<{S}, false>" if form == "chunked" else f"online_train_kernel<{S}, false> 1x1")
     for S, form in ((16, "one"), (16, "chunked"), (128, "one"), (256, "one")) for opt in ("SGD", "RMSprop")] +
    # Adam on a single-trial entry point: the captured step0 is what every replay runs with (include/mvn.h)
    [dict(id="S16-one-Adam-frozen-step0", S=16, form="one", opt="Adam", step0=5, whole_word=False, env={"MVN_TRAIN_GROUPS": "0"},
          kernel="online_train_kernel<16, false> 1x1")])
MONTECARLO = _seeded([dict(id=f"S{S}-{B}x{T}", S=S, L=L, B=B, T=T, env={}) for S, L in ((16, 4), (256, 8)) for B, T in ((37, 257), (9, 256))])


def lstm_inputs(case, rnd):
    """y [B, T + PAD] and the ten weight arrays, all new every round (the pack kernel must run on every replay)."""
    rng = _rng(case, rnd)
    y = rng.normal(0, 1.5, (case["B"], case["T"] + PAD)).astype(np.float32)
    return dict(y=y, w=[rng.uniform(-0.25, 0.25, s).astype(np.float32) for s in LSTM_SHAPES])


def step_inputs(case, rnd):
    """STEP_R words of codec_cases.batch(2, 17) (K = 120), other rows every round: rx [R, 136], tx (the messages) [R, 120]."""
    import codec_cases

    b = codec_cases.batch(STEP_NSYM, STEP_K // 8 + STEP_NSYM)
    rows = [(7 * rnd + 3 * j) % b["word"].shape[0] for j in range(STEP_R)]
    rx = codec_cases.vnet_rx(STEP_NSYM, b["n"]) if case["kind"] == "vnet" else codec_cases.clean_channel(b["word"], 0.4, seed=rnd)
    return dict(rx=np.ascontiguousarray(rx[rows]), tx=np.ascontiguousarray(b["msg"][rows]), rows=rows)


def train_inputs(case, rnd):
    """One word per round: y [T], labels int32 [T] (states below S), idx int32 [TRAIN_ITERS, TRAIN_M]."""
    rng = _rng(case, rnd)
    T = TRAIN_T
    y = rng.normal(0, 1.5, T).astype(np.float32)
    labels = rng.randint(0, case["S"], T).astype(np.int32)
    idx = np.stack([rng.choice(np.arange(1, T), TRAIN_M, replace=False) for _ in range(TRAIN_ITERS)]).astype(np.int32)
    return dict(y=y, labels=labels, idx=idx)


# ================================================== inputs, round by round =======================================================
def vnet_inputs(case, rnd):
    """dict: y [B, T + PAD], w (six arrays), tx [B, K], mask uint8 [B], rows, K -- the 16-state cases keep their weights, the
    other state counts get new ones every round and one +inf in W3 in round ODD_ROUND."""
    S, B, T = case.get("S", 16), case["B"], case["T"]
    rng = _rng(case, rnd)
    y = rng.normal(0, 1.3, (B, T + PAD)).astype(np.float32)
    if S == 16:
        w = rand_weights(S, _rng(case, 0, salt=5))
    else:
        w = rand_weights(S, _rng(case, rnd, salt=5), scale=2.0)
        w[4] *= np.float32(32.0)  # (a last layer of the untrained size decides every symbol of a 4-state block alike)
        if rnd == ODD_ROUND:
            w[4][S // 2 + 1, 11] = np.inf
    K = max(1, T - 5)
    tx = rng.randint(0, 2, (B, K)).astype(np.float32)
    rows = np.array([i for i in range(B) if i % 5 != 0], np.int64)
    mask = np.zeros(B, np.uint8)
    mask[rows] = 1
    return dict(y=y, w=w, tx=tx, mask=mask, rows=rows, K=K)


def finite_twin(w):
    """The odd round's weights with the +inf taken back (what a guard that never fired would effectively decode with)."""
    w = [a.copy() for a in w]
    w[4][~np.isfinite(w[4])] = 0.125
    return w


@functools.lru_cache(maxsize=None)
def _vnet_referee(table, idx, rnd):
    case = globals()[table][idx]
    inp = vnet_inputs(case, rnd)
    T = case["T"]
    with np.errstate(all="ignore"):
        dec, lg, fm = oracle.vnet_decode(np.ascontiguousarray(inp["y"][:, :T]), inp["w"], want_logits=True, want_final=True)
    counts = np.array(oracle.count_errors(dec[:, :inp["K"]], inp["tx"], inp["rows"]).tolist(), np.int64)
    for a in (dec, lg, fm, counts):
        a.setflags(write=False)
    return dict(dec=dec, logits=lg, final=fm, counts=counts)


def vnet_referee(case, rnd):
    table = next(t for t in ("VNET16", "VNET_STATES", "VNET_SURV", "STALE") if any(c is case for c in globals()[t]))
    return _vnet_referee(table, [c is case for c in globals()[table]].index(True), rnd)


def va_inputs(case, rnd):
    S, B, T, Bp = case["S"], case["B"], case["T"], case["Bp"]
    rng = _rng(case, rnd)
    y = rng.normal(0, 1.5, (B, T + PAD)).astype(np.float32)
    pri = rng.normal(0, 1, (Bp, S)).astype(np.float32)
    if rnd == ODD_ROUND:
        pri[Bp // 2, S // 2 + 1] = np.nan
    return dict(y=y, pri=pri)


def va_finite_twin(pri):
    pri = pri.copy()
    pri[np.isnan(pri)] = 0.125
    return pri


def va_referee(case, rnd, pri=None):
    inp = va_inputs(case, rnd)
    with np.errstate(all="ignore"):
        dec, fm = oracle.va_decode(inp["y"], inp["pri"] if pri is None else pri, T=case["T"])
    return dict(dec=dec[:, :case["T"]], final=fm)


def sweep_inputs(case, rnd):
    S, B, T = case["S"], case["B"], case["T"]
    cost = _rng(case, rnd).normal(0, 2, (B, T, S)).astype(np.float32)
    cost[B // 2] = np.round(cost[B // 2])  # exact ties
    if rnd == ODD_ROUND:  # a NaN every third block, at a different step and state each
        for b in range(0, B, 3):
            cost[b, (5 * b) % T, (3 * b) % S] = np.nan
    return cost


def sweep_finite_twin(cost):
    cost = cost.copy()
    cost[np.isnan(cost)] = 0.125
    return cost


def sweep_referee(cost):
    with np.errstate(all="ignore"):
        dec, fm = oracle.acs_sweep(cost)
    return dict(dec=dec, final=fm)


def surv_referee(cost):
    with np.errstate(all="ignore"):
        dec, fm, surv = oracle.acs_sweep_surv(cost)
        bits, states = oracle.traceback(surv, fm)
    return dict(dec=dec, final=fm, surv=surv, bits=bits, states=states)


def vnet_surv_referee(case, rnd):
    ref = vnet_referee(case, rnd)
    out = surv_referee(-ref["logits"])
    assert np.array_equal(out["final"], ref["final"])
    return out


def codec_inputs(case, rnd):
    """msg [B, 8k] fp32 bits and flip [B, 8n] fp32 {0, 1}: the bits the captured corruption inverts.  The byte positions are the
    chosen patterns of codec_cases.batch(nsym, n) with 0 ... t + 1 byte errors, dealt round-robin over the rows from a start that
    moves with the round; the error values are random and non-zero."""
    import codec_cases

    nsym, n, B = case["nsym"], case["n"], case["B"]
    k, t = n - nsym, nsym // 2
    rng = _rng(case, rnd)
    patterns = [p for p in codec_cases.batch(nsym, n)["pos"] if len(p) <= t + 1]
    msg = codec_cases.unpack(rng.randint(0, 256, (B, k)))
    err = np.zeros((B, n), np.uint8)
    n_err = np.zeros(B, np.int64)
    for r in range(B):
        pos = patterns[(r + 11 * rnd) % len(patterns)]
        n_err[r] = len(pos)
        for p in pos:
            err[r, p] = rng.randint(1, 256)
    return dict(msg=msg, flip=codec_cases.unpack(err), n_err=n_err, k=k, t=t)


def codec_referee(case, rnd):
    inp = codec_inputs(case, rnd)
    cw = oracle.rs_encode_bits(inp["msg"], case["nsym"])
    word = np.abs(cw - inp["flip"]).astype(np.float32)
    out, status = oracle.rs_decode_bits(word, case["nsym"], want_status=True)
    counts = np.array(oracle.count_errors(out, inp["msg"]).tolist(), np.int64)
    return dict(cw=cw, word=word, msg=out, status=np.asarray(status, np.int32), counts=counts)


def rows_that_differ(a, b):
    """Fraction of rows (axis 0) in which two referee outputs of the same shape differ (NaN == NaN)."""
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    return float(np.mean(~same.all(axis=1)))


# ---- the stale-flag check: what a previous replay's publication would have left in a hand-off line ------------------------------
POISON_METRICS = np.array([1000.0 * j for j in range(16)], np.float32)  # 16 finite metrics of strongly unequal size
STALE = _seeded([dict(id="rings8-1000x200", B=1000, T=200, ring=8, skip_ring=5, spin_limit=2000, env={}),
                 # (rings of one at 7000 x 100: ring 5 ends 4 symbols before its block does; ring 8 cuts its block at symbol 32)
                 dict(id="ring1-7000x100", B=7000, T=100, ring=1, skip_ring=8, spin_limit=2000, env={})])


def stale_block(case, groups=DEALT_GROUPS):
    """(block, first symbol) whose metrics ring skip_ring hands to ring skip_ring + 1: the block the skipped publication cuts."""
    U = (case["T"] + 31) // 32
    n = min(case["B"], groups) * (8 // case["ring"])
    hi = case["B"] * U * (case["skip_ring"] + 1) // n
    return hi // U, (hi % U) * 32


def publishing_ring(case, groups=DEALT_GROUPS):
    """The nearest ring below skip_ring that ends inside a block: its line holds the flag value of the launch after a replay."""
    U = (case["T"] + 31) // 32
    n = min(case["B"], groups) * (8 // case["ring"])
    return next(g for g in range(case["skip_ring"] - 1, -1, -1) if (case["B"] * U * (g + 1) // n) % U)


def continue_from(y_row, w, t0, metrics):
    """The oracle's decisions for symbols t0 ... of one block when the sweep enters t0 with path metrics `metrics`: the branch
    costs are -logit (the oracle's), the recurrence and the decision (the running argmin's low bit) the oracle's acs_block."""
    lg = oracle.vnet_logits(np.ascontiguousarray(y_row[None, :]), w)[0]
    m = np.asarray(metrics, np.float32).copy()
    out = []
    for t in range(t0, len(y_row)):
        out.append(float(np.argmin(m) % 2))  # (finite metrics here: numpy's first minimum is torch.argmin's)
        m = oracle.acs_block(m[None, :], -lg[t][None, :])[0][0]
    return np.array(out, np.float32)
