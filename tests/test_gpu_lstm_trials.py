"""GPU: the LSTM trial axis -- lstm_train_trials_kernel / lstm_maml_trials_kernel behind mvn_lstm_train_trials_f32 /
mvn_lstm_maml_train_trials_f32, the trial dimension of lstm_decode_kernel behind mvn_lstm_decode_trials_f32, LSTMTrialBank and
trials.eval_by_word_batched with an LSTM bank.  Every comparison is BITWISE against the single-trial entry points on copies of the
same state: the trials kernels run the single-trial kernels' body on a trial's own arguments, every sum has a fixed order and trials
share nothing, so nothing less is acceptable."""
import os

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm as L
from meta_viterbinet_amd import lstm_trials as LT
from test_lstm_host import g18_weights
from test_lstm_meta_host import ReplayJHat, check_g20_by_word
from test_lstm_train_host import ReplayDraws, check_g19_by_word, default_init_weights, detector_with

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NP = LT.N_PARAMS
N_ITER = (3, 0, 2, 1, 3, 2, 0, 1, 2)  # per trial: trial 1 (and 6) is idle
STEP0 = (0, 7, 0, 1023, 2, 0, 5, 1, 3)


def P():
    return int(mvn._lib.load().mvn_lstm_trials_per_launch())


def test_trials_per_launch_is_the_cu_count_over_64():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert P() == min(8, cus // 64) and P() >= 1


@pytest.fixture(scope="module")
def weight_sets():
    """Nine weight sets: default initialisations under different seeds (built once, never changed)."""
    return [default_init_weights(3 + r) for r in range(9)]


def bank_pair(weight_sets, R, optimizer_type="Adam", seed=0, M=32):
    """Two identical banks with non-trivial moments and step counts: one for the trials call, one for the single-trial calls."""
    rng = np.random.RandomState(100 + seed)
    m = torch.from_numpy((1e-3 * rng.randn(R, LT.ROW)).astype(np.float32)).to(DEV)
    v = torch.from_numpy((1e-5 * rng.rand(R, LT.ROW)).astype(np.float32)).to(DEV)
    out = []
    for _ in range(2):
        b = mvn.LSTMTrialBank(weight_sets[:R], DEV, lr=1e-3, optimizer_type=optimizer_type, train_minibatch_size=M)
        b.exp_avg.copy_(m)
        b.exp_avg_sq.copy_(v)
        b.step[:] = STEP0[:R]
        out.append(b)
    return out


def trial_inputs(R, T, M, n_iters, seed, meta=False):
    """Per trial: its own number of words, the words, the word of every iteration and the minibatch positions (training) or the
    support and query words of every step (meta-learning); device tensors."""
    rng = np.random.RandomState(7 * T + seed)
    ins = []
    for r in range(R):
        nw = 2 + (r % 3) if meta else 1 + ((r + 2) % 3)
        bits = rng.randint(0, 2, (nw, T))
        rx = ((1 - 2 * bits) + 0.4 * rng.randn(nw, T)).astype(np.float32)
        n = max(n_iters[r], 1)
        d = dict(n_words=nw, bits=torch.from_numpy(bits.astype(np.int32)).to(DEV), rx=torch.from_numpy(rx).to(DEV),
                 woi=torch.from_numpy(rng.randint(0, nw, n).astype(np.int32)).to(DEV),
                 idx=torch.from_numpy(rng.randint(0, T, (n, max(M, 1))).astype(np.int32)).to(DEV),
                 loss=torch.full((n,), -1.0, device=DEV), loss_ref=torch.full((n,), -1.0, device=DEV))
        if not meta and r % 4 == 2:
            d["woi"] = None  # online training: word 0 in every iteration
        ins.append(d)
    return ins


def single_trial_calls(bank, ins, n_iters, T, M, meta=False, meta_lr=0.1):
    """The reference: one mvn_lstm_train_f32 / mvn_lstm_maml_train_f32 call per trial with n_iter > 0 on the rows of `bank`."""
    lib, ptr = mvn._lib.load(), mvn._lib.ptr
    ws = torch.empty(int(lib.mvn_lstm_maml_workspace_bytes(T)), dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    b1, b2, eps = bank.kernel_optimizer_args()
    for r, d in enumerate(ins):
        if n_iters[r] == 0:
            continue
        w = [ptr(t) for t in bank.weights(r)]
        if meta:
            rc = lib.mvn_lstm_maml_train_f32(ptr(d["rx"]), T, ptr(d["bits"]), T, d["n_words"], ptr(d["idx"]), ptr(d["woi"]), n_iters[r], *w,
                                             ptr(bank.exp_avg[r]), ptr(bank.exp_avg_sq[r]), int(bank.step[r]), meta_lr, bank.lr, b1, b2, eps,
                                             ptr(d["loss_ref"]), ptr(ws), ws.numel(), ptr(status), T, mvn._lib.current_stream(DEV))
        else:
            rc = lib.mvn_lstm_train_f32(ptr(d["rx"]), T, ptr(d["bits"]), T, d["n_words"], ptr(d["woi"]), ptr(d["idx"]) if M else None, M,
                                        n_iters[r], *w, ptr(bank.exp_avg[r]), ptr(bank.exp_avg_sq[r]), int(bank.step[r]), bank.lr, b1, b2, eps,
                                        ptr(d["loss_ref"]), ptr(ws), ws.numel(), ptr(status), T, mvn._lib.current_stream(DEV))
        assert rc == 0
        bank.step[r] += n_iters[r]
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def trials_call(bank, ins, n_iters, T, M, meta=False, meta_lr=0.1):
    R = len(ins)
    p = lambda key: [None if d[key] is None else d[key].data_ptr() for d in ins]  # noqa: E731
    if meta:  # a step's support word is idx[k, 0], its query word woi[k]
        bank.maml_trials(list(range(R)), p("rx"), p("bits"), [d["n_words"] for d in ins], p("idx"), p("woi"), n_iters, T, meta_lr,
                         loss_out=p("loss"))
    else:
        bank.train_trials(list(range(R)), p("rx"), p("bits"), [d["n_words"] for d in ins], n_iters, T, M, p("idx"), p("woi"), p("loss"))
    torch.cuda.synchronize()
    bank.check_status()
    assert not bank.status.any()


def u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def assert_banks_equal(a, b, ins, n_iters, start=None):
    for name in ("theta", "exp_avg", "exp_avg_sq", "saved"):
        assert np.array_equal(u32(getattr(a, name)), u32(getattr(b, name))), name
    assert np.array_equal(a.step, b.step)
    for r, d in enumerate(ins):
        assert np.array_equal(u32(d["loss"]), u32(d["loss_ref"])), r
        if n_iters[r]:
            assert torch.isfinite(d["loss"]).all() and torch.isfinite(a.theta[r]).all()
            if start is not None:
                assert not torch.equal(a.theta[r], start.theta[r])  # it trained
        else:  # an idle trial: nothing of it was written
            assert float(d["loss"][0]) == -1.0
            if start is not None:
                assert all(torch.equal(getattr(a, n)[r], getattr(start, n)[r]) for n in ("theta", "exp_avg", "exp_avg_sq"))


def compare_training(weight_sets, R, T, M, optimizer_type="Adam", n_iters=N_ITER, meta=False):
    n_iters = list(n_iters[:R])
    a, b = bank_pair(weight_sets, R, optimizer_type, seed=R)
    start = bank_pair(weight_sets, R, optimizer_type, seed=R)[0]
    ins = trial_inputs(R, T, M, n_iters, seed=R, meta=meta)
    if meta:
        for d in ins:  # support words [n] in column 0 of idx, another draw than the query words
            d["idx"] = torch.from_numpy(np.random.RandomState(T + d["n_words"]).randint(0, d["n_words"], d["idx"].shape[0]).astype(np.int32)).to(DEV)
    trials_call(a, ins, n_iters, T, M, meta)
    single_trial_calls(b, ins, n_iters, T, M, meta)
    assert_banks_equal(a, b, ins, n_iters, start)


@pytest.mark.parametrize("M", [0, 4])
@pytest.mark.parametrize("T", [1, 5, 37])
def test_training_trials_equal_sequential_single_trial_calls(weight_sets, T, M):
    """R = 1, 2, P and P + 1 trials (the last: a second launch) with different words, positions, iteration counts (one trial idle)
    and step numbers: parameters, both moments and the losses of every trial bit for bit those of mvn_lstm_train_f32."""
    if M > T:
        M = T
    for R in sorted({1, 2, P(), P() + 1}):
        compare_training(weight_sets, R, T, M)


@pytest.mark.parametrize("optimizer_type,T,M", [("RMSprop", 5, 4), ("SGD", 37, 0), ("Adam", 37, 4)])
def test_training_trials_every_optimizer(weight_sets, optimizer_type, T, M):
    compare_training(weight_sets, 3, T, M, optimizer_type)


def test_training_trials_split_over_launches_by_the_switch(weight_sets):
    """MVN_LSTM_TRIALS_PER_LAUNCH=2 and three running trials: two launches, the same bits; a value above CUs / 64 is clamped."""
    lib = mvn._lib.load()
    before = P()
    try:
        os.environ["MVN_LSTM_TRIALS_PER_LAUNCH"] = "2" if before >= 2 else "1"
        lib.mvn_reload_switches()
        assert P() == min(2, before)
        compare_training(weight_sets, 3, 5, 4, n_iters=(3, 2, 1))
        os.environ["MVN_LSTM_TRIALS_PER_LAUNCH"] = "8"
        lib.mvn_reload_switches()
        assert P() == before
    finally:
        os.environ.pop("MVN_LSTM_TRIALS_PER_LAUNCH", None)
        lib.mvn_reload_switches()
    assert P() == before


def test_one_trial_of_two_past_a_launchs_iteration_limit(weight_sets):
    """n_iter = (8193, 3) at T = 1: the first trial continues in a second launch (step0, word_of_iter and loss_out advanced) while
    the second has finished; equal to the single-trial calls."""
    compare_training(weight_sets, 2, 1, 0, n_iters=(8193, 3))


@pytest.mark.parametrize("T", [2, 37])
def test_meta_learning_trials_equal_sequential_single_trial_calls(weight_sets, T):
    """R = P + 1 trials, (2, 0, 3, 1, 2, ...) steps, a different n_words and different support and query words per trial."""
    compare_training(weight_sets, P() + 1, T, 0, n_iters=(2, 0, 3, 1, 2, 1, 0, 2, 1), meta=True)


@pytest.mark.parametrize("T", [1, 5, 136])
@pytest.mark.parametrize("B", [1, 17])
def test_detection_trials_equal_single_trial_calls(weight_sets, B, T):
    R = 5
    bank = mvn.LSTMTrialBank(weight_sets[:R], DEV)
    assert bank.theta.stride(0) == 795140
    rng = np.random.RandomState(10 * B + T)
    big = torch.from_numpy(rng.randn(R * B, T + 3).astype(np.float32)).to(DEV)
    y = big.as_strided((R, B, T), (B * (T + 3), T + 3, 1))  # row-strided (T + 3 floats apart), read in place
    dec, logits = mvn.lstm_decode_trials(y, bank, return_logits=True)
    assert dec.shape == (R, B, T) and logits.shape == (R, B, T, 2)
    seen = set()
    for r in range(R):
        d1, l1 = L.lstm_decode(y[r], bank.weights(r), return_logits=True)
        assert torch.equal(dec[r], d1) and np.array_equal(u32(logits[r]), u32(l1)), r
        seen.add(l1.cpu().numpy().tobytes())
    assert len(seen) == R  # the trials' weights differ, and so do their logits
    assert torch.equal(mvn.lstm_decode_trials(y.contiguous(), bank), dec)


# ---------------------------------------------------------------------------------------------------------------------------
# by word
# ---------------------------------------------------------------------------------------------------------------------------
def sequential_run(ws, tx, rx, draws, kw, lr=1e-3):
    """harness.eval_by_word alone on one trial: (ser, trained blocks, meta blocks, trainer, saved weights or None)."""
    det = detector_with(ws, DEV)
    tr = mvn.LSTMMetaTrainer(det, lr=lr)
    trained, metas, last = [], [], {}

    def observer(seen):
        last.update(seen)
        if seen["stage"] == "end" and seen["trained"]:
            trained.append(seen["count"])
        if seen["stage"] == "meta":
            metas.append(seen["count"])

    ser = mvn.eval_by_word(det, tx, rx, 10.0, 0.2, online_trainer=tr, draws=draws, observer=observer, **kw)
    saved = last.get("saved_detector")
    return ser, trained, metas, tr, None if saved is None else torch.cat([p.detach().reshape(-1) for p in saved._params()])


def assert_row_equals_sequential(bank, r, ser_row, record, seq, with_saved=False):
    ser, trained, metas, tr, saved = seq
    assert np.array_equal(ser_row, ser)
    assert np.flatnonzero(record["trained"][r]).tolist() == trained and np.flatnonzero(record["meta"][r]).tolist() == metas
    assert np.array_equal(u32(bank.theta[r, :NP]), u32(torch.cat([p.detach().reshape(-1) for p in tr.params])))
    assert np.array_equal(u32(bank.exp_avg[r, :NP]), u32(tr.exp_avg)) and np.array_equal(u32(bank.exp_avg_sq[r, :NP]), u32(tr.exp_avg_sq))
    assert int(bank.step[r]) == tr.step
    if with_saved:
        assert saved is not None and np.array_equal(u32(bank.saved[r, :NP]), u32(saved))


def other_frame_order(a, sub):
    """The same blocks with the frames (a pilot and its data blocks) rotated by one; a single frame: its data blocks reversed."""
    n = a.shape[0] // sub
    if n >= 2:
        return np.concatenate([a[sub:], a[:sub]])
    return np.concatenate([a[:1], a[1:][::-1]])


def test_by_word_g19_three_trials(golden):
    """G19 (c): 50 blocks, 8 minibatch iterations per trained block.  Trial 0 is the golden run, trial 1 starts from a default
    initialisation (it seldom trains: the idle-trial path), trial 2 sees the frames in another order with its own draws."""
    g19, g18 = golden("g19_lstm_train"), golden("g18_lstm")
    iters, sub, nsym, _, _ = [int(v) for v in g19["c_meta"]]
    txs = [g19["c_tx"], g19["c_tx"], other_frame_order(g19["c_tx"], sub)]
    rxs = [g19["c_rx"], g19["c_rx"], other_frame_order(g19["c_rx"], sub)]
    tx = torch.from_numpy(np.stack(txs).astype(np.float32)).to(DEV)
    rx = torch.from_numpy(np.stack(rxs)).to(DEV)
    wss = [g18_weights(g18), default_init_weights(), g18_weights(g18)]
    make_draws = lambda: [ReplayDraws(g19["c_idx"]), mvn.TrialDraws(11, DEV), mvn.TrialDraws(12, DEV)]  # noqa: E731
    kw = dict(n_symbols=nsym, subframes_in_frame=sub, self_supervised=True, self_supervised_iterations=iters,
              ser_thresh=float(g19["c_ser_thresh"]))
    bank = mvn.LSTMTrialBank(wss, DEV)
    record = {}
    ser = mvn.eval_by_word_batched(bank, tx, rx, draws=make_draws(), record=record, **kw)
    assert ser.shape == (3, tx.shape[1])
    check_g19_by_word(g19, ser[0], np.flatnonzero(record["trained"][0]).tolist())
    counts = [int(record["trained"][r].sum()) for r in range(3)]
    print(f"trained blocks per trial: {counts}")
    assert counts[0] == len(g19["c_trained"]) and counts[1] < counts[0]
    for r, d in enumerate(make_draws()):
        assert_row_equals_sequential(bank, r, ser[r], record, sequential_run(wss[r], tx[r], rx[r], d, kw))
        assert int(bank.step[r]) == iters * counts[r]


def test_by_word_g20_two_trials_meta_learning(golden):
    """G20 (c): 25 blocks, first-order meta updates and whole-word training from the saved weights; trial 1 sees the data blocks
    in another order with its own j_hat draws."""
    g20, g18 = golden("g20_lstm_meta"), golden("g18_lstm")
    ss_iters, sub, nsym, _, _, meta_iters, meta_j, meta_sub = [int(v) for v in g20["c_meta"]]
    tx = torch.from_numpy(np.stack([g20["c_tx"], other_frame_order(g20["c_tx"], sub)]).astype(np.float32)).to(DEV)
    rx = torch.from_numpy(np.stack([g20["c_rx"], other_frame_order(g20["c_rx"], sub)])).to(DEV)
    wss = [g18_weights(g18), g18_weights(g18)]
    make_draws = lambda: [ReplayJHat(g20["c_randint_high"], g20["c_randint"]), mvn.TrialDraws(21, DEV)]  # noqa: E731
    kw = dict(n_symbols=nsym, subframes_in_frame=sub, self_supervised=True, self_supervised_iterations=ss_iters,
              ser_thresh=float(g20["c_ser_thresh"]), online_meta=True, meta_lr=float(g20["c_meta_lr"]), MAML=False, window_size=1,
              meta_train_iterations=meta_iters, meta_j_num=meta_j, meta_subframes=meta_sub, meta_style_online_training=True,
              weights_init="last_frame")
    bank = mvn.LSTMTrialBank(wss, DEV)
    record = {}
    ser = mvn.eval_by_word_batched(bank, tx, rx, draws=make_draws(), record=record, **kw)
    check_g20_by_word(g20, ser[0], np.flatnonzero(record["trained"][0]).tolist(), np.flatnonzero(record["meta"][0]).tolist(),
                      [w.cpu().numpy() for w in bank.weights(0)])
    assert record["meta"][1].sum() >= 1
    for r, d in enumerate(make_draws()):
        assert_row_equals_sequential(bank, r, ser[r], record, sequential_run(wss[r], tx[r], rx[r], d, kw), with_saved=True)


def test_by_word_hand_off_route(golden):
    """window_size = 2 is not the lock-step engine's: trial after trial through harness.eval_by_word (autograd meta steps), the
    same results as running it yourself, and the bank's state written back.  Two meta steps per trial."""
    g20, g18 = golden("g20_lstm_meta"), golden("g18_lstm")
    sub, nsym = int(g20["c_meta"][1]), int(g20["c_meta"][2])
    N = 11
    tx = torch.from_numpy(np.stack([g20["c_tx"][:N], other_frame_order(g20["c_tx"][:N], N)]).astype(np.float32)).to(DEV)
    rx = torch.from_numpy(np.stack([g20["c_rx"][:N], other_frame_order(g20["c_rx"][:N], N)])).to(DEV)
    wss = [g18_weights(g18), g18_weights(g18)]
    kw = dict(n_symbols=nsym, subframes_in_frame=sub, ser_thresh=1.0, online_meta=True, meta_lr=0.1, MAML=False, window_size=2,
              meta_train_iterations=1, meta_j_num=1, meta_subframes=5, weights_init="last_frame")
    assert not LT.lock_step_serves(rx.shape[2], True, False, 2)
    bank = mvn.LSTMTrialBank(wss, DEV)
    start = bank.theta.clone()
    record = {}
    ser = mvn.eval_by_word_batched(bank, tx, rx, draws=[mvn.TrialDraws(31, DEV), mvn.TrialDraws(32, DEV)], record=record, **kw)
    for r in range(2):
        seq = sequential_run(wss[r], tx[r], rx[r], mvn.TrialDraws(31 + r, DEV), kw)
        assert seq[2] == [5, 10] and seq[3].step == 2
        assert_row_equals_sequential(bank, r, ser[r], record, seq, with_saved=True)
        assert not torch.equal(bank.theta[r], start[r]) and torch.equal(bank.saved[r], bank.theta[r])
