"""Evaluation harness for the detection hot path: counterpart of Trainer.single_eval_at_point /
gamma_eval / eval_by_word's detector calls (python_code/trainers/trainer.py:222-265, 292-295), plus the
block-parallel multi-GPU Monte-Carlo loop the reference does not have.

Blocks (words) are independent, so the batch axis is split contiguously across ranks; every rank
decodes its rows, counts errors on the device as integers, and ONE all_reduce(SUM) of an int64[4]
tensor {bit_errors, bits, frame_errors, frames} (RCCL over xGMI when backend='nccl') ends the run.
Decisions are never gathered.  Integer counters make 1/2/4/8-GPU results identical."""
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import metrics as _metrics
from .channel import estimate_channel, transmit
from .ecc import list_step_bytes, rs_decode, rs_encode
from .trellis import calculate_states


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous split of n rows: rank r owns [lo, hi); sizes differ by at most one."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def data_indices(val_frames: int, subframes_in_frame: int) -> torch.Tensor:
    """Non-pilot rows: every row whose index is not a multiple of subframes_in_frame (trainer.py:100-102)."""
    idx = [i for i in range(val_frames * subframes_in_frame) if i % subframes_in_frame != 0]
    return torch.tensor(idx, dtype=torch.int64)


def synthetic_words(n_words: int, block_length: int, memory_length: int, snr: float, gamma: float,
                    device, seed: int, channel_coefficients: str = "time_decay", fused: bool = True):
    """At-scale synthetic inputs generated on `device`: bits ~ Bernoulli(1/2), zero-padded by
    L, BPSK 1-2c, anti-causal ISI y[t] = sum_k h[L-1-k] s[t+k] + w[t] (channel.py:25-27), w ~ N(0, 10^(-snr/10)).
    Same distribution as ChannelModelDataset (channel_dataset.py:55-95), different RNG stream.
    On a GPU the words come from ONE kernel (channel.generate_words: Philox bits + Box-Muller noise + the L-tap channel);
    fused=False keeps the older route (ATen randint / randn + mvn_isi_awgn_transmit).
    Returns (tx [n,block_length] fp32 {0,1}, y [n,block_length] fp32)."""
    L = memory_length
    h = estimate_channel(L, gamma, channel_coefficients)
    if fused and torch.device(device).type == "cuda":
        from .channel import generate_words

        return generate_words(n_words, block_length, h, snr, L, device, seed)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    tx = torch.randint(0, 2, (n_words, block_length), generator=g, device=device, dtype=torch.int8).to(torch.float32)
    noise = torch.randn(n_words, block_length, generator=g, device=device)
    if torch.device(device).type == "cuda":
        return tx, transmit(tx, h, snr, L, noise)  # mvn_isi_awgn_transmit
    # CPU (host-side tests only): the same arithmetic in torch float64
    s = 1.0 - 2.0 * torch.cat([tx, torch.zeros(n_words, L)], dim=1).double()
    y = torch.zeros(n_words, block_length, dtype=torch.float64)
    for i in range(L):
        y += float(h[0, L - 1 - i]) * s[:, i:i + block_length]
    y += ((10 ** (snr / 10)) ** (-0.5)) * noise.double()
    return tx, y.float()


def va_monte_carlo(detector, n_words: int, snr: float, gamma: float, device, seed: int, counters: Optional[torch.Tensor] = None):
    """One uncoded Monte-Carlo point of the classical Viterbi detector in ONE launch (mvn_va_montecarlo_f32): what
    Trainer.single_eval_at_point does (trainer.py:222-241: draw the words, detector(rx, 'val'), calculate_error_rates), with the words
    of synthetic_words(..., seed) generated inside the detector and compared there -- no tx, y or decisions in device memory (at
    BASELINE configs[3], 10^6 blocks x 1000 symbols, those are 12 GB).  16 or 256 states; the words' channel is the detector's
    (`_estimate_all`: row b % val_words for word b, like its state priors).  Returns int64[4] counters {bit_errors, bits,
    frame_errors, frames} on `device` (accumulated into `counters` when given): the same numbers as
    count_errors(detector(y, 'val', snr, gamma), tx) over (tx, y) = synthetic_words(n_words, T, L, snr, gamma, device, seed)."""
    from . import _lib

    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.MvnError("va_monte_carlo runs on an MI355X (ROCm) device only")
    T, L, S = detector.transmission_length, detector.memory_length, detector.n_states
    h = torch.as_tensor(np.ascontiguousarray(detector._estimate_all(gamma, "val"), dtype=np.float64).reshape(-1, L), device=dev)
    pri = detector._priors_table(torch.empty(0, device=dev), gamma, "val", None)
    if counters is None:
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
    sigma = (10 ** (snr / 10)) ** (-0.5)  # channel.py:23,31
    with torch.cuda.device(dev):
        rc = _lib.load().mvn_va_montecarlo_f32(_lib.ptr(h), h.shape[0], float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(pri),
                                               pri.shape[0], _lib.ptr(counters), n_words, T, L, S, _lib.current_stream(dev))
    _lib.check(rc, "mvn_va_montecarlo_f32")
    return counters


def vnet_monte_carlo(detector, n_words: int, h, snr: float, device, seed: int, counters: Optional[torch.Tensor] = None,
                     first_word: int = 0, rounds: int = 1, stop_frame_errors: int = 0):
    """One uncoded Monte-Carlo point of the 16-state ViterbiNet with the words generated INSIDE the detector
    (mvn_vnet_montecarlo_f32): Trainer.single_eval_at_point (trainer.py:222-241) with no tx, y or decisions in device memory.
    `detector`: a 16-state VNETDetector (its weights are read at call time); T = detector.transmission_lengths['val'], L = 4.
    `h`: estimate_channel(...) rows [Bh, 4] (ViterbiNet carries no channel of its own; an array, or a float64 tensor already on
    `device`); word w uses row w % Bh.
    Returns the int64[4] counters {bit_errors, bits, frame_errors, frames} on `device` (accumulated into `counters` when given): the
    same numbers as detector.val_count(y, tx) over rows first_word : first_word + n_words of
    (tx, y) = generate_words(first_word + n_words, T, h, snr, 4, device, seed).

    rounds = R > 1 runs R rounds of n_words words each (round r: words first_word + r n_words ...), all enqueued at once;
    stop_frame_errors = F > 0 lets a round run only if fewer than F frame errors had been counted when the round before it
    completed -- the run-to-F-frame-errors form of a BER/FER point, decided on the device between the rounds: the call never
    synchronises, a round runs whole or not at all, and the same arguments give the same integers every time.  With rounds > 1
    the call returns (counters, rounds_run), rounds_run an int32 device tensor (read it when the counters are read).

    Sharding a point over ranks: words are addressed globally, so rank r of `world` calls
    lo, hi = shard_range(n_total, r, world); vnet_monte_carlo(det, hi - lo, h, snr, device, seed, first_word=lo) and the ranks
    all_reduce(SUM) the counters as sharded_eval does -- 1, 2, 4 or 8 ranks give identical integers.  (With rounds, a rank's round r
    starts at first_word + r n_words: give every rank its own contiguous range of rounds * n_words words.)"""
    from . import _lib

    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.MvnError("vnet_monte_carlo runs on an MI355X (ROCm) device only")
    S, L = detector.n_states, 4
    T = detector.transmission_lengths["val"]
    if n_words < 0 or rounds < 0 or first_word < 0 or stop_frame_errors < 0:
        raise ValueError("n_words, rounds, first_word and stop_frame_errors must not be negative")
    from .detectors import _weights_on

    if torch.is_tensor(h):
        hd = h.to(device=dev, dtype=torch.float64).reshape(-1, L).contiguous()
    else:
        hd = torch.as_tensor(np.ascontiguousarray(h, dtype=np.float64).reshape(-1, L), device=dev)
    w = _weights_on(detector._params(), dev, S)  # read at call time, never cached
    if counters is None:
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
    staged = rounds > 1 or stop_frame_errors > 0
    progress = torch.zeros(2, dtype=torch.int32, device=dev) if staged else None
    sigma = (10 ** (snr / 10)) ** (-0.5)  # channel.py:23,31
    with torch.cuda.device(dev):
        rc = _lib.load().mvn_vnet_montecarlo_f32(_lib.ptr(hd), hd.shape[0], float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, first_word,
                                                 *[_lib.ptr(t) for t in w], _lib.ptr(counters), _lib.ptr(progress), n_words, rounds,
                                                 stop_frame_errors, T, L, S, _lib.current_stream(dev))
    _lib.check(rc, "mvn_vnet_montecarlo_f32")
    return (counters, progress[0]) if rounds > 1 else counters


def _gpu_counter(detected: torch.Tensor, tx: torch.Tensor, rows: Optional[torch.Tensor]) -> torch.Tensor:
    return _metrics.count_errors(detected, tx, rows)


DECISIONS = ("running", "path")


def _check_decision(decision: str, detector=None, by_word: bool = False) -> None:
    """decision: 'running' = the reference's running argmin (quirk Q1, symbol t decided before stage t is absorbed), 'path' = the
    traced-back maximum-likelihood word (detector.viterbi_path); the LSTM detectors have no trellis to trace back.
    'list' (by_word: eval_by_word only) = the path's word, list-decoded in the one-launch block step (ecc.list_decode)."""
    if decision == "list":
        if not by_word:
            raise ValueError("decision='list' exists in the by-word block step only (eval_by_word, eval_by_word_batched); "
                             "to decode a batch of words call list_decode(detector, rx, n_symbols)")
        if not hasattr(detector, "viterbi_path"):
            raise ValueError(f"decision='list' needs a Viterbi / ViterbiNet detector ({type(detector).__name__} has no trellis)")
        return
    if decision not in DECISIONS:
        raise ValueError(f"decision must be one of {DECISIONS + ('list',) if by_word else DECISIONS}, got {decision!r}")
    if decision == "path" and not hasattr(detector, "viterbi_path"):
        raise ValueError(f"decision='path' needs a Viterbi / ViterbiNet detector ({type(detector).__name__} has no viterbi_path)")


def _detect(detector: Callable, y: torch.Tensor, snr: float, gamma: float, decision: str = "running", count: int = None,
            pass_count: bool = False) -> torch.Tensor:
    """detector(y, 'val', snr, gamma[, count]), or its traced-back path for decision='path'."""
    if decision == "path":
        from .detectors import VADetector

        if not isinstance(detector, VADetector):  # ViterbiNet's path takes the word only (its forward ignores snr, gamma, count)
            return detector.viterbi_path(y)
        return detector.viterbi_path(y, snr, gamma, count) if pass_count else detector.viterbi_path(y, snr, gamma)
    return detector(y, "val", snr, gamma, count) if pass_count else detector(y, "val", snr, gamma)


def eval_counters(detector: Callable, tx: torch.Tensor, rx: torch.Tensor, snr: float, gamma: float,
                  rows: Optional[torch.Tensor] = None, counter: Callable = _gpu_counter,
                  group=None, reduce: bool = True, n_symbols: int = 0, rs_decoder: Callable = rs_decode,
                  decision: str = "running") -> torch.Tensor:
    """One Monte-Carlo point on THIS rank's rows: detect -> [RS decode] -> count -> (optionally) all-reduce.
    `tx`/`rx` are the rank-local shards; `rows` are local row indices counted (None = all).
    n_symbols > 0 = the reference's use_ecc path (trainer.py:234-236): detected words are RS-decoded (on the
    device) before they are compared with the transmitted message bits.
    decision='path': the traced-back word (detector.viterbi_path) is counted instead of the running-argmin decisions.
    Returns int64[4] counters (global sums when reduce=True and a process group is up)."""
    _check_decision(decision, detector)
    if n_symbols > 0:
        detected = _detect(detector, rx, snr, gamma, decision)
        counters = counter(rs_decoder(detected, n_symbols)[:, : tx.shape[1]], tx, rows)
    elif decision == "path":
        counters = counter(_detect(detector, rx, snr, gamma, decision)[:, : tx.shape[1]], tx, rows)
    elif counter is _gpu_counter and getattr(detector, "n_states", None) == 16 and hasattr(detector, "val_count"):
        counters = detector.val_count(rx, tx, rows)  # decode + count in one launch, decisions never stored
    else:
        detected = detector(rx, "val", snr, gamma)
        counters = counter(detected[:, : tx.shape[1]], tx, rows)
    if reduce and dist.is_available() and dist.is_initialized():
        dist.all_reduce(counters, op=dist.ReduceOp.SUM, group=group)
    return counters


def single_eval_at_point(detector: Callable, tx: torch.Tensor, rx: torch.Tensor, snr: float, gamma: float,
                         rows: Optional[torch.Tensor] = None, counter: Callable = _gpu_counter,
                         group=None, n_symbols: int = 0, decision: str = "running") -> Tuple[float, float, torch.Tensor]:
    """trainer.py:222-241 without the data draw: detect, optional RS decode (n_symbols > 0 = use_ecc), error
    rates over the data rows.  Returns (ser, fer, counters); the reference returns ser only (:238-241)."""
    counters = eval_counters(detector, tx, rx, snr, gamma, rows, counter, group, n_symbols=n_symbols, decision=decision)
    ser, fer = _metrics.rates_from_counters(counters)
    return ser, fer, counters


def sharded_eval(detector: Callable, tx: torch.Tensor, rx: torch.Tensor, snr: float, gamma: float,
                 rows: Optional[torch.Tensor] = None, counter: Callable = _gpu_counter, group=None,
                 rank: Optional[int] = None, world: Optional[int] = None, n_symbols: int = 0,
                 rs_decoder: Callable = rs_decode, decision: str = "running") -> Tuple[float, float, torch.Tensor]:
    """Same point, but given the FULL (tx, rx) on every rank: each rank takes its contiguous row shard
    (shard_range), maps the global `rows` filter into it, and the counters are all-reduced."""
    if rank is None:
        rank = dist.get_rank(group) if dist.is_initialized() else 0
    if world is None:
        world = dist.get_world_size(group) if dist.is_initialized() else 1
    lo, hi = shard_range(tx.shape[0], rank, world)
    local_rows = None
    if rows is not None:
        r = rows.to("cpu")
        r = r[(r >= lo) & (r < hi)] - lo
        local_rows = r.to(tx.device)
    if hi > lo:
        counters = eval_counters(detector, tx[lo:hi], rx[lo:hi], snr, gamma, local_rows, counter, group, reduce=False,
                                 n_symbols=n_symbols, rs_decoder=rs_decoder, decision=decision)
    else:
        counters = torch.zeros(4, dtype=torch.int64, device=tx.device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(counters, op=dist.ReduceOp.SUM, group=group)
    ser, fer = _metrics.rates_from_counters(counters)
    return ser, fer, counters


def replica_eval(trial: Callable, n_trials: int, group=None, rank: Optional[int] = None,
                 world: Optional[int] = None, device=None, batched: bool = False) -> np.ndarray:
    """Replica mode for the evaluations that do NOT shard within a trial: with online training
    between blocks (eval_by_word with self_supervised / online_meta, trainer.py:292-347) block k's weights depend on the
    blocks before it, so one trial stays on one GPU and the parallel axis is the (SNR x seed x method) grid the reference
    walks serially (plotters/plotter_main.py:117-149).  Rank r runs trials r, r + world, ...; `trial(i)` returns that
    trial's float ser_by_word vector (all trials the same length); ONE all_gather of the float32 vectors (1.2 KB per
    trial) ends the run.  Returns [n_trials, N] (row i = trial i) on every rank.
    batched=True: `trial` takes the LIST of this rank's trial numbers and returns their vectors as rows [len(list), N] --
    the rank's trials then advance together on its GPU (trials.eval_by_word_batched) instead of one after the other.
    `device`: where the gathered tensor lives (a CUDA device under backend 'nccl' = RCCL, 'cpu' under gloo)."""
    up = dist.is_available() and dist.is_initialized()
    if rank is None:
        rank = dist.get_rank(group) if up else 0
    if world is None:
        world = dist.get_world_size(group) if up else 1
    ids = list(range(rank, n_trials, world))
    if batched:
        rows = np.asarray(trial(ids), dtype=np.float32).reshape(len(ids), -1) if ids else np.zeros((0, 0), np.float32)
        mine = [rows[k] for k in range(len(ids))]
    else:
        mine = [np.asarray(trial(i), dtype=np.float32).reshape(-1) for i in ids]
    per_rank = (n_trials + world - 1) // world
    n = mine[0].shape[0] if mine else 0
    if up and world > 1:  # ranks without a trial still need the vector length for the collective
        nt = torch.tensor([n], dtype=torch.int64, device=device if device is not None else "cpu")
        dist.all_reduce(nt, op=dist.ReduceOp.MAX, group=group)
        n = int(nt.item())
    local = torch.full((per_rank, n), float("nan"), dtype=torch.float32)
    for k, v in enumerate(mine):
        local[k] = torch.from_numpy(v)
    if not (up and world > 1):
        return local[:n_trials].numpy()
    local = local.to(device if device is not None else "cpu")
    gathered = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(gathered, local, group=group)
    out = np.empty((n_trials, n), np.float32)
    for r, g in enumerate(gathered):
        g = g.cpu().numpy()
        for k, i in enumerate(range(r, n_trials, world)):
            out[i] = g[k]
    return out


def detect_by_word(detector: Callable, rx: torch.Tensor, snr: float, gamma: float, batched: bool = True,
                   pass_count: bool = False) -> torch.Tensor:
    """The detector calls of eval_by_word (trainer.py:292-295) when no online update runs between blocks
    ("joint" variant): block k's decision does not depend on blocks < k, so the 300 B=1 calls collapse
    into one batched call (batched=True) -- or are issued one by one exactly like the reference."""
    if batched and not pass_count:
        return detector(rx, "val", snr, gamma)
    outs = []
    for count in range(rx.shape[0]):
        word = rx[count].reshape(1, -1)
        outs.append(detector(word, "val", snr, gamma, count) if pass_count else detector(word, "val", snr, gamma))
    return torch.cat(outs, dim=0)


def eval_by_word(detector, tx: torch.Tensor, rx: torch.Tensor, snr: float, gamma: float, n_symbols: int,
                 subframes_in_frame: int, self_supervised: bool = False, online_trainer=None,
                 self_supervised_iterations: int = 200, ser_thresh: float = 0.02, pass_count: bool = False,
                 verbose: bool = False, online_meta: bool = False, meta_detector=None, meta_lr: float = 0.1,
                 MAML: bool = True, window_size: int = 1, meta_train_iterations: int = 20, meta_j_num: int = 10,
                 meta_subframes: int = 5, meta_style_online_training: bool = False,
                 graphed_meta: bool = True, hip_meta: bool = True, initial_buffer=None, weights_init: str = "last_frame",
                 meta_training_weights=None, draws=None, fused_step: bool = True, observer=None,
                 decision: str = "running", list_bytes: Optional[int] = None) -> np.ndarray:
    """Sequential per-block online evaluation: counterpart of Trainer.eval_by_word (trainer.py:267-354).  Everything but the
    control flow stays on the GPU:
        for every block k:  detect (B=1)  ->  data block: RS decode, ser, RS re-encode | pilot: encode the known word
            ->  if ser <= ser_thresh: buffer (rx, label), label = detected word if ser > 0 else the re-encoded word
            ->  if online_meta and k % meta_subframes == 0 (k >= meta_subframes, buffer > 2): restart from the saved
                weights, meta_train_iterations x {meta_j_num random (support, query) pairs of consecutive buffered words ->
                meta.meta_train_loop}, save the weights (:331-343)
            ->  if self_supervised (and ser <= ser_thresh): online_trainer.online_training(last buffered pair) (:345-347);
                meta_style_online_training=True first restores the saved weights and trains on the whole word
                (metavnet_trainer.py:52-64), otherwise a 32-sample minibatch per iteration (vnet_trainer.py:49-60).
    initial_buffer = (tx_codewords [W, T], rx_words [W, T]): the reference's buffer_empty=False (:278-286) -- the buffer
    starts with W words drawn from the training channel and stays W long (every qualifying block pushes the oldest out,
    :325-328); None = buffer_empty=True.  weights_init (meta_weights_init, :356-366): what a meta update restarts from --
    'last_frame' the weights saved after the previous update, 'random' freshly initialised weights and a fresh optimizer,
    'meta_training' the weights in `meta_training_weights` (the reference loads its meta-trained checkpoint).
    tx [N, K] message bits, rx [N, K + 8*n_symbols] received words; block k is a pilot when k % subframes_in_frame == 0
    (trainer.py:100-102).  Returns ser_by_word [N] (0 for pilots), like the reference.
    One host sync per block (the ser decides what happens next), as in the reference (trainer.py:305).
    draws: a trials.TrialDraws -- the minibatches and j_hat values come from this trial's own streams instead of the global
    generators (the reference's are unseeded), which is what makes a run replayable inside trials.eval_by_word_batched.
    fused_step: a 16-state ViterbiNet detector with nsym <= 8 takes ONE launch per block (mvn_vnet_byword_step_f32:
    detect, RS decode, error count, re-encode); False keeps the four separate launches (the cross-check in the tests).
    So does a ViterbiNet detector at 4, 8, 32, 64 or 128 states with the running decision (mvn_vnet_byword_step_states_f32) and with
    decision='path' (mvn_vnet_byword_step_states_path_f32), words up to _lib.step_max_symbols(n_states) symbols.
    observer: called at the end of every block of the update branches with a dict {stage: 'end', count, ser, pushed,
    buffer_rx, buffer_tx, meta: (support_idx [n, W], query_idx [n]) or None, trained, batch_idx, detector, saved_detector},
    and with stage 'meta' right after a meta-learning update launched by the HIP kernel: what a test needs to replay the
    block's updates on another implementation (tests/test_gpu_replay.py).
    An LSTMDetector with online_trainer=LSTMMetaTrainer(detector) runs the same branches as the Meta-LSTM curve
    (meta_lstm_trainer.py): meta_detector defaults to MetaLSTMDetector(), every meta update is ONE maml_training call (first order
    with window_size 1: one launch of mvn_lstm_maml_train_f32; otherwise the trainer's autograd route), graphed_meta does not apply,
    weights_init='random' re-initialises the detector in place like LSTMDetector() and resets the optimizer, and
    meta_style_online_training=True is MetaLSTMTrainer.online_training.
    decision: 'running' (default) detects like the reference, by the running argmin (quirk Q1); 'path' detects every block by the
    traced-back maximum-likelihood word -- in the one-launch step where it applies (mvn_vnet_byword_step_path_f32 /
    mvn_va_byword_step_path_f32), else by detector.viterbi_path in the separate launches -- and everything downstream (RS
    decode, ser, the buffered label word, every update branch) runs unchanged on it.  Not for the LSTM detectors (ValueError).
    decision='list': the path's word, decoded by the reliability-ordered list decoder in the same launch
    (mvn_vnet_byword_step_list_f32 / mvn_va_byword_step_list_f32; list_bytes = how many least reliable bytes the erasure patterns
    are drawn from, default n_symbols + 2): the message is the candidate the trellis likes best, and the error count, the re-encoded
    word and the buffered label word follow from it.  It exists in the one-launch step only: ValueError when the step's conditions
    (_fused_step_applies, fused_step=True) or T <= 512 do not hold.  A ViterbiNet detector at 4, 8, 32, 64 or 128 states takes
    mvn_vnet_byword_step_states_list_f32 (_states_list_step_applies: the path step's conditions and words up to
    _lib.list_max_symbols(n_states) symbols).  A VADetector at 4, 8, 32, 64 or 128 states takes mvn_va_byword_step_states_f32, _path_f32
    and _list_f32 under the 16-state VA rule (_va_states_step_applies: words up to _lib.va_step_max_symbols(n_states), for 'list'
    _lib.va_list_max_symbols(n_states), symbols); 2 and 256 states have no list step.  At 256 states either detector takes
    mvn_{vnet,va}_byword_step_256_f32 / _256_path_f32 for 'running' and 'path' (_step256_applies: the 16-state rules, words up to
    _lib.step256_max_symbols() / _lib.va_step256_max_symbols() symbols)."""
    import copy

    from .meta import GraphedMetaStep, copy_model, meta_train_loop

    from .lstm import LSTMDetector, LSTMMetaTrainer, LSTMOnlineTrainer, MetaLSTMDetector

    _check_decision(decision, detector, by_word=True)
    lstm_meta = False  # the Meta-LSTM curve: an LSTMDetector meta-learned by an LSTMMetaTrainer (meta_lstm_trainer.py)
    if isinstance(detector, (LSTMDetector, MetaLSTMDetector)):
        if online_meta:
            if not (isinstance(detector, LSTMDetector) and isinstance(online_trainer, LSTMMetaTrainer)):
                raise ValueError("eval_by_word: meta-learning of an LSTMDetector needs online_trainer=LSTMMetaTrainer(detector) "
                                 "(meta_lstm_trainer.py)")
            lstm_meta = True
            if meta_detector is None:
                meta_detector = MetaLSTMDetector()
        if (self_supervised or online_trainer is not None) and not (isinstance(detector, LSTMDetector)
                                                                    and isinstance(online_trainer, LSTMOnlineTrainer)):
            raise ValueError("eval_by_word: online training of an LSTMDetector needs online_trainer=LSTMOnlineTrainer(detector) "
                             "(lstm_trainer.py, meta_lstm_trainer.py)")
    elif isinstance(online_trainer, LSTMOnlineTrainer):
        raise ValueError("eval_by_word: an LSTMOnlineTrainer trains an LSTMDetector")
    N = tx.shape[0]
    ser_by_word = np.zeros(N)
    K = tx.shape[1]
    va_states = fused_step and _va_states_step_applies(detector, rx, n_symbols, pass_count, decision)  # a VADetector off 16 states
    step256 = fused_step and _step256_applies(detector, rx, n_symbols, pass_count, decision)  # either detector at 256 states
    fused = step256 or va_states or (fused_step and (_fused_step_applies(detector, rx, n_symbols, pass_count, decision)
                                          or (decision == "list" and _states_list_step_applies(detector, rx, n_symbols, pass_count))))
    if decision == "list":
        if not va_states:
            _va_states_list_conditions(detector, rx, n_symbols, pass_count, fused_step)
        list_bytes = (list_step_bytes(rx.shape[1], n_symbols, list_bytes) if va_states else
                      _list_step_bytes(detector, rx, n_symbols, pass_count, fused_step, list_bytes))
    elif list_bytes is not None:
        raise ValueError("list_bytes belongs to decision='list'")
    step = _block_step(detector, rx.shape[1], n_symbols, decision, list_bytes) if fused else None
    if not (self_supervised or online_meta or verbose):
        # No update runs between blocks, so nothing on the host depends on a block's ser: the reference's 300 B=1 detector
        # calls are issued one by one like it issues them, but the per-block error counts stay on the device and ONE
        # transfer ends the run (the reference synchronises after every block, trainer.py:305).  Pilot blocks are skipped:
        # their ser is 0 and their detection only feeds the buffer of the update branches.
        if fused:  # one launch per data block: detect + RS decode + error count (+ the re-encoding nobody reads here)
            nerr = torch.zeros(N, dtype=torch.int32, device=rx.device)
            for count in range(N):
                if count % subframes_in_frame != 0:
                    _byword_step(step, detector, rx[count:count + 1], tx[count:count + 1], False, nerr[count:count + 1],
                                 outputs=False, gamma=gamma, count=count if pass_count else None)
            e = nerr.cpu().numpy()
            data = np.arange(N) % subframes_in_frame != 0
            ser_by_word[data] = _metrics.ser_from_errors(e[data], K)  # the reference's value bit for bit (metrics.py:13-16)
            return ser_by_word
        counters = torch.zeros((N, 4), dtype=torch.int64, device=rx.device)  # row k: {bit errors, bits, ...} of block k
        for count in range(N):
            if count % subframes_in_frame == 0:
                continue
            received_word = rx[count:count + 1]
            detected_word = _detect(detector, received_word, snr, gamma, decision, count, pass_count)
            _metrics.count_errors(rs_decode(detected_word, n_symbols), tx[count:count + 1], None, counters[count])
        c = counters.cpu().numpy()
        data = c[:, 1] > 0
        ser_by_word[data] = _metrics.ser_from_errors(c[data, 0], K)  # the reference's value bit for bit (metrics.py:13-16)
        return ser_by_word
    if (self_supervised or online_meta) and online_trainer is None:
        raise ValueError("self_supervised / online_meta need an OnlineTrainer (it owns the Adam state)")
    if weights_init not in ("last_frame", "random", "meta_training"):
        raise ValueError("No such weights init!!!")
    if weights_init == "meta_training" and meta_training_weights is None:
        raise ValueError("weights_init='meta_training' needs meta_training_weights (the arrays in parameters() order)")
    if online_meta and meta_detector is None:
        raise ValueError("online_meta needs a META_VNETDetector")
    saved_detector = copy.deepcopy(detector) if (online_meta or meta_style_online_training) else None  # :275
    buffer_empty = initial_buffer is None
    if buffer_empty:
        buffer_rx = torch.empty([0, rx.shape[1]], device=rx.device)
        buffer_tx = torch.empty([0, rx.shape[1]], device=rx.device)
    else:
        buffer_tx, buffer_rx = [t.to(device=rx.device, dtype=torch.float32) for t in initial_buffer]
    meta_step = None  # meta.GraphedMetaStep, built at the first meta update (graphed_meta and a CUDA detector)
    graphed_meta = graphed_meta and rx.is_cuda and (online_trainer is None or online_trainer.optimizer_type == "Adam")  # captured Adam update
    # mvn_vnet_maml_train_f32: n_states <= 128 (4 parameter vectors in LDS up to 32 states, 2 at 64 / 128); the kernel's optimizer is Adam
    if lstm_meta:
        # every step of an update in ONE LSTMMetaTrainer.maml_training call, which takes the kernel (first order, one support word:
        # one launch) or autograd by its own meta_kernel_route; nothing is captured into a graph
        graphed_meta, hip_meta = False, True
    else:
        hip_meta = (hip_meta and online_meta and rx.is_cuda and detector.n_states <= 128 and online_trainer is not None
                    and online_trainer.optimizer_type == "Adam" and online_trainer.use_kernel)
    support_idx = torch.arange(-window_size - 1, -1, device=rx.device).long()  # :288
    query_idx = -1 * torch.ones(1, device=rx.device).long()

    def draw_j_hat(high):  # trainer.py:337: the global generator, or this trial's own stream
        if draws is None:
            return torch.unique(torch.randint(low=0, high=high, size=[meta_j_num])).to(rx.device)
        return torch.as_tensor(draws.j_hat(high, meta_j_num), device=rx.device).long()

    from .detectors import VNETDetector

    # The fused ViterbiNet step also picks the word the reference buffers and computes its trellis states (what the training
    # kernels take as labels), and the block's error count travels to the host together with the trainer's status word: one
    # launch and one 8-byte copy per block before the host decides.
    # (the step's states are those of the detector's own trellis, memory length log2 n_states)
    step_labels = (fused and isinstance(detector, VNETDetector) and online_trainer is not None and online_trainer.use_kernel
                   and 2 ** online_trainer.memory_length == detector.n_states)
    sync_words = online_trainer.sync_words if (step_labels and getattr(online_trainer, "sync_words", None) is not None) else None
    nerr1 = (sync_words[:1] if sync_words is not None else torch.zeros(1, dtype=torch.int32, device=rx.device)) if fused else None
    buffer_lab = None
    if step_labels:
        buffer_lab = (torch.empty([0, rx.shape[1]], dtype=torch.int32, device=rx.device) if buffer_empty else
                      calculate_states(online_trainer.memory_length, buffer_tx).reshape(buffer_tx.shape).to(torch.int32))
    for count in range(N):
        transmitted_word, received_word = tx[count].reshape(1, -1), rx[count].reshape(1, -1)
        pilot = count % subframes_in_frame == 0
        seen = {"count": count, "meta": None, "trained": False, "batch_idx": None} if observer is not None else None
        status_word = None
        if step_labels:  # ONE launch: detect, RS decode, error count, re-encode, the word to buffer and its states
            label_word, label_states = _byword_step(step, detector, received_word, transmitted_word, pilot, nerr1, labels=True)
            if sync_words is not None:
                n_err, status_word = sync_words.tolist()
            else:
                n_err = int(nerr1.item())
            ser = 0.0 if pilot else float(_metrics.ser_from_errors(n_err, K))  # calculate_error_rates (:301)
            if not pilot:
                ser_by_word[count] = ser
        elif fused:  # ONE launch: detect, RS decode, error count, re-encode (pilot: encode the known word)
            detected_word, encoded_word = _byword_step(step, detector, received_word, transmitted_word, pilot, nerr1,
                                                       gamma=gamma, count=count if pass_count else None)
            ser = 0.0 if pilot else float(_metrics.ser_from_errors(int(nerr1.item()), K))  # calculate_error_rates (:301)
            if not pilot:
                ser_by_word[count] = ser
        else:
            detected_word = _detect(detector, received_word, snr, gamma, decision, count, pass_count)
            if not pilot:
                decoded_word = rs_decode(detected_word, n_symbols)
                ser = float(_metrics.ser_from_errors(int((decoded_word != transmitted_word).sum().item()), K))  # calculate_error_rates (:301)
                encoded_word = rs_encode(decoded_word, n_symbols)  # :304
                ser_by_word[count] = ser
            else:
                encoded_word = rs_encode(transmitted_word, n_symbols)  # pilot: the word is known (:314-316)
                ser = 0.0
        if online_trainer is not None:
            online_trainer.check_status(status_word)  # a training launch that gave up its barrier (NaN weights) raises here
        if verbose:
            print(f"current: {count, ser}")
        if ser <= ser_thresh:  # :319-329 (buffer_empty=True: the buffer only grows)
            buffer_rx = torch.cat([buffer_rx, received_word])
            if step_labels:
                buffer_tx = torch.cat([buffer_tx, label_word], dim=0)
                buffer_lab = torch.cat([buffer_lab, label_states], dim=0)
            else:
                buffer_tx = torch.cat([buffer_tx, detected_word.reshape(1, -1) if ser > 0 else encoded_word.reshape(1, -1)], dim=0)
            if not buffer_empty:  # fixed-length window: the oldest word leaves (:325-328)
                buffer_rx, buffer_tx = buffer_rx[1:], buffer_tx[1:]
                if step_labels:
                    buffer_lab = buffer_lab[1:].contiguous()
        if online_meta and count % meta_subframes == 0 and count >= meta_subframes and buffer_rx.shape[0] > 2:  # :331-343
            if weights_init == "last_frame":  # meta_weights_init (:356-366)
                copy_model(source_model=saved_detector, dest_model=detector)
            elif weights_init == "random":
                if lstm_meta:  # initialize_detector (meta_lstm_trainer.py:26-30): what LSTMDetector() draws, in place
                    detector.lstm.reset_parameters()
                    detector.fc.reset_parameters()
                elif draws is not None:  # this trial's own stream (what lets trials.eval_by_word_batched replay the run)
                    with torch.no_grad():
                        for p_, w_ in zip(detector.parameters(), draws.init_weights(detector.n_states)):
                            p_.copy_(w_)
                else:
                    for m in detector.net:
                        if hasattr(m, "reset_parameters"):
                            m.reset_parameters()
                online_trainer.reset_state()
            else:
                with torch.no_grad():
                    for p_, w_ in zip(detector.parameters(), meta_training_weights):
                        p_.copy_(torch.as_tensor(w_, dtype=p_.dtype))
            if hip_meta:  # every MAML step of this update in ONE launch of the meta-learning kernel
                if draws is not None:  # the update's j_hat values in one draw (this trial's own stream)
                    j_all = torch.as_tensor(draws.j_hat_update(buffer_rx.shape[0] - 2, meta_train_iterations, meta_j_num),
                                            device=rx.device).long()
                else:
                    j_all = torch.cat([draw_j_hat(buffer_rx.shape[0] - 2) for _ in range(meta_train_iterations)])
                sup_all = j_all.reshape(-1, 1) + support_idx.reshape(1, -1) + 1
                qry_all = j_all + query_idx + 1
                online_trainer.maml_training(buffer_rx, buffer_tx, sup_all, qry_all, meta_lr, MAML, labels=buffer_lab)
                if seen is not None:
                    seen["meta"] = (sup_all, qry_all)
            else:
                if graphed_meta and meta_step is None:  # captured once: one hipGraph replay per MAML step from here on
                    meta_step = GraphedMetaStep(detector, meta_detector, online_trainer, window_size, rx.shape[1], meta_lr,
                                                MAML)
                j_seen = []
                for _ in range(meta_train_iterations):
                    j_hat_values = draw_j_hat(buffer_rx.shape[0] - 2)
                    j_seen.append(j_hat_values)
                    for j_hat in j_hat_values:
                        if meta_step is not None:
                            meta_step(buffer_rx, buffer_tx, j_hat + support_idx + 1, j_hat + query_idx + 1)
                        else:
                            meta_train_loop(detector, meta_detector, online_trainer, buffer_rx, buffer_tx,
                                            j_hat + support_idx + 1, j_hat + query_idx + 1, meta_lr, MAML)
                if seen is not None:
                    j_all = torch.cat(j_seen)
                    seen["meta"] = (j_all.reshape(-1, 1) + support_idx.reshape(1, -1) + 1, j_all + query_idx + 1)
            copy_model(source_model=detector, dest_model=saved_detector)
            if seen is not None and seen["meta"] is not None:
                observer(dict(seen, stage="meta", detector=detector, saved_detector=saved_detector, buffer_rx=buffer_rx,
                              buffer_tx=buffer_tx))
        if self_supervised and ser <= ser_thresh:  # :345-347
            if meta_style_online_training:
                copy_model(source_model=saved_detector, dest_model=detector)  # metavnet_trainer.py:59
            batch_idx = None
            if draws is not None and not meta_style_online_training:
                batch_idx = draws.batches(count, N, rx.shape[1], self_supervised_iterations, online_trainer.train_minibatch_size)
            if seen is not None and batch_idx is None and not meta_style_online_training:
                batch_idx = online_trainer.select_batches(rx.shape[1], self_supervised_iterations)  # drawn here to be shown
            online_trainer.online_training(buffer_tx[-1].reshape(1, -1), buffer_rx[-1].reshape(1, -1),
                                           iterations=self_supervised_iterations, batch_idx=batch_idx,
                                           full_word=meta_style_online_training,
                                           labels=None if buffer_lab is None else buffer_lab[-1])
            if seen is not None:
                seen.update(trained=True, batch_idx=batch_idx)
        if seen is not None:
            seen.update(stage="end", ser=ser, pushed=ser <= ser_thresh, buffer_rx=buffer_rx, buffer_tx=buffer_tx, detector=detector,
                        saved_detector=saved_detector)
            observer(seen)
    if online_trainer is not None:
        online_trainer.check_status()
    return ser_by_word


def _fused_step_applies(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool, decision: str = "running") -> bool:
    """One launch per block step (mvn_vnet_byword_step_f32 / mvn_va_byword_step_f32) serves a 16-state VNETDetector or
    VADetector whose 'val' length is the word length (Q5), words of whole bytes up to 1024 symbols and nsym <= 8; everything
    else takes the separate detect / RS / count launches.  (pass_count: the reference passes the block number to the detector,
    which is how VADetector picks the word's channel; ViterbiNet ignores it.)
    A VNETDetector at 4, 8, 32, 64 or 128 states has the step for the running decision (mvn_vnet_byword_step_states_f32) and for the
    traced-back path (mvn_vnet_byword_step_states_path_f32), for words up to _lib.step_max_symbols(n_states) symbols; 'list' is a
    16-state step."""
    from . import _lib
    from .detectors import VADetector, VNETDetector

    T = rx.shape[1]
    S = getattr(detector, "n_states", None)
    if not (rx.is_cuda and T % 8 == 0 and 8 <= T <= 1024 and 1 <= n_symbols <= 8 and T // 8 > n_symbols):
        return False
    if S != 16:
        return (S in _lib.STEP_STATES and isinstance(detector, VNETDetector) and decision in ("running", "path") and not pass_count
                and detector.transmission_lengths["val"] == T and T <= _lib.step_max_symbols(S))
    if isinstance(detector, VNETDetector):
        return not pass_count and detector.transmission_lengths["val"] == T
    # VADetector: the fused step takes ONE row of state priors -- the word's own (pass_count) or the table's only row.  A
    # multi-row table without the block number takes the separate launches, where the detector itself raises what the
    # reference raises (the [1, S] / [W, S] broadcast of va_detector.py:64-68).
    return isinstance(detector, VADetector) and detector.transmission_length == T and (pass_count or detector.val_words == 1)


def _states_list_step_applies(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool) -> bool:
    """decision='list' off 16 states: a VNETDetector at 4, 8, 32, 64 or 128 states under the path step's conditions
    (_fused_step_applies) takes mvn_vnet_byword_step_states_list_f32 for words up to _lib.list_max_symbols(n_states) symbols."""
    from . import _lib

    S = getattr(detector, "n_states", None)
    return (S in _lib.STEP_STATES and _fused_step_applies(detector, rx, n_symbols, pass_count, "path")
            and rx.shape[1] <= _lib.list_max_symbols(S))


def _va_states_step_applies(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool, decision: str = "running") -> bool:
    """A VADetector at 4, 8, 32, 64 or 128 states takes one launch per block step (mvn_va_byword_step_states_f32, _path_f32, _list_f32)
    under the 16-state VA rule of _fused_step_applies: the detector's length is the word length, ONE row of state priors (the word's
    own with pass_count, or the table's only row), words of whole bytes longer than the parity, nsym 1 ... 8, and T within the rule's
    longest word (_lib.va_step_max_symbols / _lib.va_list_max_symbols).  Consulted BEFORE _fused_step_applies,
    _states_list_step_applies and _list_step_bytes, which keep answering for such a detector what they answered before this step
    existed.  eval_by_word takes the step by default at every one of these state counts: it measured faster than the separate launches
    at each, for 'running' and for 'path' (profiles/va_states_step_time.txt); 'list' has no other route."""
    from . import _lib
    from .detectors import VADetector

    T = rx.shape[1]
    S = getattr(detector, "n_states", None)
    if not (isinstance(detector, VADetector) and S in _lib.STEP_STATES and decision in ("running", "path", "list")):
        return False
    if not (rx.is_cuda and T % 8 == 0 and T >= 8 and 1 <= n_symbols <= 8 and T // 8 > n_symbols):
        return False
    if not (detector.transmission_length == T and (pass_count or detector.val_words == 1)):
        return False
    return T <= (_lib.va_list_max_symbols(S) if decision == "list" else _lib.va_step_max_symbols(S))


# The detector / decision pairs of the 256-state step that eval_by_word takes by default: those that measured faster than the separate
# launches at R = 1 (profiles/states256_step_time.txt).  A pair that is False keeps its entry point and BywordStep(states_256=True).
_STEP256_DEFAULT = {("vnet", "running"): True, ("vnet", "path"): True, ("va", "running"): True, ("va", "path"): True}


def _step256_applies(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool, decision: str = "running") -> bool:
    """A VNETDetector or a VADetector at 256 states (channel memory 8) takes one launch per block step (mvn_vnet_byword_step_256_f32 /
    _256_path_f32, mvn_va_byword_step_256_f32 / _256_path_f32) under the 16-state rules of _fused_step_applies: words of whole bytes
    longer than the parity, nsym 1 ... 8; ViterbiNet: the 'val' length is the word length and no block number is passed; VA: the
    detector's length is the word length and ONE row of state priors (the word's own with pass_count, or the table's only row); T
    within the step's longest word (_lib.step256_max_symbols / _lib.va_step256_max_symbols).  'list' has no step at 256 states.
    Consulted BEFORE _va_states_step_applies, _fused_step_applies, _states_list_step_applies and _list_step_bytes, which keep
    answering for a 256-state detector what they answered before this step existed."""
    from . import _lib
    from .detectors import VADetector, VNETDetector

    T = rx.shape[1]
    if getattr(detector, "n_states", None) != 256 or decision not in ("running", "path"):
        return False
    if not (rx.is_cuda and T % 8 == 0 and T >= 8 and 1 <= n_symbols <= 8 and T // 8 > n_symbols):
        return False
    if isinstance(detector, VNETDetector):
        return (_STEP256_DEFAULT["vnet", decision] and not pass_count and detector.transmission_lengths["val"] == T
                and T <= _lib.step256_max_symbols())
    if isinstance(detector, VADetector):
        return (_STEP256_DEFAULT["va", decision] and detector.transmission_length == T and (pass_count or detector.val_words == 1)
                and T <= _lib.va_step256_max_symbols())
    return False


def _va_states_list_conditions(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool, fused_step: bool) -> None:
    """decision='list' with a VADetector at 4, 8, 32, 64 or 128 states that _va_states_step_applies turned down: the ValueError that
    names the condition (there is no other route to fall back to).  Every other detector: nothing (_list_step_bytes speaks for it)."""
    from . import _lib
    from .detectors import VADetector

    S = getattr(detector, "n_states", None)
    if not (isinstance(detector, VADetector) and S in _lib.STEP_STATES and rx.is_cuda and fused_step):
        return
    T = rx.shape[1]
    list_step_bytes(T, n_symbols, None)
    if T > _lib.va_list_max_symbols(S):
        raise ValueError(f"decision='list' serves words of up to {_lib.va_list_max_symbols(S)} symbols at {S} states with a VADetector "
                         f"(branch costs, forward metrics and survivors stay in LDS), got T = {T}")
    if detector.transmission_length != T:
        raise ValueError(f"decision='list': the detector's transmission_length {detector.transmission_length} is not the word length {T}")
    if not (pass_count or detector.val_words == 1):
        raise ValueError("decision='list': a VADetector with several rows of state priors needs pass_count=True")


def _list_step_bytes(detector, rx: torch.Tensor, n_symbols: int, pass_count: bool, fused_step: bool, list_bytes) -> int:
    """decision='list' exists in the one-launch block step only: the validated list_bytes, or a ValueError that names the
    condition that does not hold (there is no other route to fall back to)."""
    from . import _lib
    from .detectors import VADetector, VNETDetector

    T = rx.shape[1]
    m = list_step_bytes(T, n_symbols, list_bytes)
    if not fused_step:
        raise ValueError("decision='list' runs in the one-launch block step: fused_step=False has no list decoder")
    if not rx.is_cuda:
        raise ValueError("decision='list' needs the received words on an MI355X (ROCm) device")
    S = getattr(detector, "n_states", None)
    if S in _lib.STEP_STATES and isinstance(detector, VNETDetector):
        if T > _lib.list_max_symbols(S):
            raise ValueError(f"decision='list' serves words of up to {_lib.list_max_symbols(S)} symbols at {S} states (logits, forward "
                             f"metrics and survivors stay in LDS), got T = {T}")
    elif S != 16:
        raise ValueError("decision='list' needs a 16-state detector, or a ViterbiNet detector at 4, 8, 32, 64 or 128 states")
    if isinstance(detector, VNETDetector):
        if pass_count:
            raise ValueError("decision='list': a ViterbiNet detector takes no block number (pass_count=False)")
        if detector.transmission_lengths["val"] != T:
            raise ValueError(f"decision='list': the detector's 'val' length {detector.transmission_lengths['val']} is not the word length {T}")
    elif isinstance(detector, VADetector):
        if detector.transmission_length != T:
            raise ValueError(f"decision='list': the detector's transmission_length {detector.transmission_length} is not the word length {T}")
        if not (pass_count or detector.val_words == 1):
            raise ValueError("decision='list': a VADetector with several rows of state priors needs pass_count=True")
    else:
        raise ValueError(f"decision='list' needs a VNETDetector or a VADetector, not {type(detector).__name__}")
    assert _fused_step_applies(detector, rx, n_symbols, pass_count) if S == 16 else _states_list_step_applies(detector, rx, n_symbols, pass_count)
    return m


def _block_step(detector, T: int, n_symbols: int, decision: str, list_bytes):
    """The detector's one-launch block step for this run (resolved once, before the block loop)."""
    from . import _lib
    from .detectors import VADetector

    return _lib.BywordStep("va" if isinstance(detector, VADetector) else "vnet", decision, T, n_symbols, list_bytes,
                           n_states=detector.n_states, states_path=True, states_list=True, states_va=True, states_256=True)


def _byword_step(step, detector, received_word: torch.Tensor, transmitted_word: torch.Tensor, pilot: bool, nerr: torch.Tensor,
                 outputs: bool = True, gamma: float = None, count: int = None, labels: bool = False):
    """One block of eval_by_word in one launch (trainer.py:292-316; step: _block_step's): returns (detected_word, encoded_word)
    [1, T]; the block's bit-error count goes to nerr[0] (device int32).  On a pilot the detection is skipped (never used) and
    detected_word is None.  outputs=False: the error count only (no words are stored, the re-encoding is skipped).
    gamma / count: what VADetector.forward takes to find the word's channel (count None: the detector's single table row).
    labels=True (ViterbiNet): returns (label_word [1, T], states int32 [1, T]) instead -- the word the reference pushes into its
    buffer (:322-324: the detected word if it had bit errors, else the re-encoded one) and its trellis states, both chosen and
    computed by the kernel.  The step's decision 'path': the same step on the traced-back word (the *_path_f32 entry points);
    'list': that step with the list decoder (the *_list_f32 entry points, list_bytes least reliable bytes)."""
    from . import _lib
    from .detectors import VADetector

    rxw, txw = _lib.f32c(received_word), _lib.f32c(transmitted_word)
    T, K = rxw.shape[1], txw.shape[1]
    dev = rxw.device
    if isinstance(detector, VADetector):
        pri = detector._priors_table(rxw, gamma, "val", count)  # [W, n_states] (one row when count is given)
        assert pri.shape[0] == 1  # (_fused_step_applies / _va_states_step_applies send every other table to the separate launches)
        front = (_lib.ptr(pri), 1)
    else:
        front = (*[_lib.ptr(_lib.f32c(p)) for p in detector._params()], None)
    if labels:
        got = (torch.empty((1, T), dtype=torch.float32, device=dev), torch.empty((1, T), dtype=torch.int32, device=dev))
        out = {"label_word": (_lib.ptr(got[0]), T), "labels": (_lib.ptr(got[1]), T)}
    else:
        got = (None if (pilot or not outputs) else torch.empty((1, T), dtype=torch.float32, device=dev),
               torch.empty((1, T), dtype=torch.float32, device=dev) if outputs else None)
        out = {"dec": (_lib.ptr(got[0]), T), "enc": (_lib.ptr(got[1]), T)} if outputs else {}
    step(dev, _lib.ptr(rxw), T, _lib.ptr(txw), K, front, out, _lib.ptr(nerr), 1, pilot)
    return got


# ---- the two offline loops that produce the weights every evaluation above starts from: Trainer.train() (trainer.py:455-490) and
# Trainer.meta_train() (trainer.py:383-423), for one SNR each
class JointTrainResult(NamedTuple):
    losses: np.ndarray        # [n_minibatches] float64: the steps' losses of a minibatch summed like `current_loss +=` (trainer.py:479)
    ser: np.ndarray           # [n_minibatches] float64: single_eval_at_point's ser after each minibatch
    best_ser: float
    best_weights: list        # six tensors (parameters() order): the copy kept by the strict `ser < best_ser` (trainer.py:485-487)
    best_minibatch: int       # 0-based
    step_losses: np.ndarray   # [n_minibatches, steps] float32
    counters: np.ndarray      # [n_minibatches, 4] int64 {bit_errors, bits, frame_errors, frames} of each validation


class MetaTrainResult(NamedTuple):
    losses: np.ndarray        # [n_minibatches] float64: the query losses of a minibatch summed (trainer.py:416)
    ser: np.ndarray           # [n_minibatches] float64
    weights: list             # per minibatch the six tensors saved after it (save_weights runs every minibatch, trainer.py:423)
    step_losses: list         # per minibatch float32 [steps]: one per j_hat value
    counters: np.ndarray      # [n_minibatches, 4] int64
    j_hat: list               # per minibatch the int64 j_hat values used


def reference_word_source(memory_length: int, device, snr: float, gamma: float, block_length: int = 120, n_symbols: int = 0,
                          train_frames: int = 12, val_frames: int = 12, subframes_in_frame: int = 25,
                          channel_coefficients: str = "time_decay", noisy_est_var: float = 0, fading_in_channel: bool = False,
                          fading_in_decoder: bool = False, fading_taps_type: int = 1, noise_seed: int = 3450002,
                          word_seed: int = 7860002) -> Callable:
    """words(minibatch, phase) for joint_train / meta_train: the two datasets of initialize_dataloaders (trainer.py:187-217) on ONE
    channel.ReferenceWordStream -- the reference's datasets share their two RandomState streams, so 'train' and 'val' draws continue
    one sequence in call order.  'train': frames * subframes words through time_decay taps, fading = fading_in_decoder; 'val': the
    configured channel_coefficients, fading = fading_in_channel; word i of a draw uses estimate_channel(..., index=i)
    (channel_dataset.py:55-85).  Returns (b [n, block_length] message bits, y [n, block_length + 8 n_symbols]), on the device."""
    from .channel import ReferenceWordStream

    stream = ReferenceWordStream(block_length, memory_length, device, n_symbols, noise_seed, word_seed)
    n = {"train": train_frames * subframes_in_frame, "val": val_frames * subframes_in_frame}
    coeff = {"train": "time_decay", "val": channel_coefficients}
    fading = {"train": fading_in_decoder, "val": fading_in_channel}

    def words(minibatch: int, phase: str):
        h = np.concatenate([estimate_channel(memory_length, gamma, coeff[phase], noisy_est_var, fading[phase], i, fading_taps_type)
                            for i in range(n[phase])], axis=0)
        return stream.draw(n[phase], h, snr)

    return words


def _word_source(words, word_source, detector, online_trainer, snr, gamma, n_symbols, subframes_in_frame) -> Callable:
    """The caller's words(minibatch, phase), or reference_word_source on the detector's device with the trainer's memory length;
    word_source: further keyword arguments of reference_word_source (block_length, train_frames, val_frames, the channel's
    settings, the two seeds)."""
    if words is not None:
        if word_source:
            raise ValueError("word_source holds the settings of the default word source: give it or `words`, not both")
        return words
    return reference_word_source(online_trainer.memory_length, next(detector.parameters()).device, snr, gamma, n_symbols=n_symbols,
                                 subframes_in_frame=subframes_in_frame, **(word_source or {}))


def _params_copy(detector) -> list:
    return [p.detach().clone() for p in detector.parameters()]


def _validation(detector, tx, rx, snr, gamma, rows, n_symbols, evaluate):
    """(ser, counters int64[4] on the host) of one validation draw: single_eval_at_point (trainer.py:222-241), or the caller's
    evaluate(detector, tx, rx) -> (ser, counters)."""
    if evaluate is not None:
        ser, counters = evaluate(detector, tx, rx)
    else:
        ser, _, counters = single_eval_at_point(detector, tx, rx, snr, gamma, rows, n_symbols=n_symbols)
    return float(ser), np.asarray(torch.as_tensor(counters).cpu(), dtype=np.int64).reshape(4)


def joint_train(detector, online_trainer, snr: float, gamma: float, n_minibatches: int, words: Optional[Callable] = None,
                n_symbols: int = 0, subframes_in_frame: int = 25, batch_idx=None, full_word: bool = False,
                evaluate: Optional[Callable] = None, word_source: Optional[dict] = None, verbose: bool = False) -> JointTrainResult:
    """The body of Trainer.train() for one SNR (trainer.py:468-489) on `detector` as it stands (the reference initialises detector and
    optimizer just before, :466-467: pass a fresh VNETDetector and OnlineTrainer).  For each of n_minibatches:
        tx, rx = words(minibatch, 'train')              the minibatch's training words: tx [n, K] message bits, rx [n, T]
        online_trainer.train_words(tx, rx, ...)         one optimizer step per word, in ONE launch on the kernel route (:476-479)
        tx, rx = words(minibatch, 'val') -> ser         single_eval_at_point over the data rows (:482; n_symbols > 0 = use_ecc)
        ser < best_ser: keep a copy of the weights      (:485-487; strict, and the first minibatch always wins against inf)
    words: a callable (minibatch number from 0, 'train' | 'val') -> (tx, rx), e.g. one that replays recorded words; None: the
    reference's own source, reference_word_source(**word_source) (channel.ReferenceWordStream with the 'train' / 'val' settings of
    initialize_dataloaders; it transmits on the device).  batch_idx: the select_batch draws -- None: online_trainer.select_batches(K, n) per minibatch; an array
    [n_minibatches, n, M] of recorded draws; or a callable minibatch -> [n, M].  full_word=True: every step uses the whole word.
    evaluate(detector, tx, rx) -> (ser, counters [4]): replaces single_eval_at_point (a CPU detector has no 'val' path here).
    The data rows of a validation are those whose number is no multiple of subframes_in_frame (trainer.py:100-102)."""
    words = _word_source(words, word_source, detector, online_trainer, snr, gamma, n_symbols, subframes_in_frame)
    best_ser, best_weights, best_minibatch = float("inf"), None, -1
    losses, sers, step_losses, counters = [], [], [], []
    for mb in range(n_minibatches):
        tx, rx = words(mb, "train")
        idx = None
        if not full_word and batch_idx is not None:
            idx = torch.as_tensor(np.asarray(batch_idx(mb) if callable(batch_idx) else batch_idx[mb]))
        loss = online_trainer.train_words(tx, rx, batch_idx=idx, full_word=full_word, return_loss=True)
        vtx, vrx = words(mb, "val")
        rows = torch.tensor([i for i in range(vtx.shape[0]) if i % subframes_in_frame != 0], dtype=torch.int64, device=vtx.device)
        ser, cnt = _validation(detector, vtx, vrx, snr, gamma, rows, n_symbols, evaluate)
        if hasattr(online_trainer, "check_status"):
            online_trainer.check_status()
        sl = loss.detach().cpu().numpy().astype(np.float32)
        step_losses.append(sl)
        current_loss = 0.0
        for v in sl:  # `current_loss += loss.item()` (trainer.py:479)
            current_loss += float(v)
        losses.append(current_loss)
        sers.append(ser)
        counters.append(cnt)
        if verbose:
            print(f"Minibatch {mb + 1}, ser - {ser}, loss {current_loss}")
        if ser < best_ser:
            best_ser, best_weights, best_minibatch = ser, _params_copy(detector), mb
    return JointTrainResult(np.asarray(losses), np.asarray(sers), best_ser, best_weights, best_minibatch,
                            np.stack(step_losses) if step_losses else np.zeros((0, 0), np.float32),
                            np.stack(counters) if counters else np.zeros((0, 4), np.int64))


def meta_train(detector, meta_detector, online_trainer, snr: float, gamma: float, n_minibatches: int,
               words: Optional[Callable] = None, n_symbols: int = 0, subframes_in_frame: int = 25, window_size: int = 1,
               meta_j_num: int = 10, meta_lr: float = 0.1, MAML: bool = True, j_hat=None, evaluate: Optional[Callable] = None,
               encode: Optional[Callable] = None, word_source: Optional[dict] = None, verbose: bool = False) -> MetaTrainResult:
    """The body of Trainer.meta_train() for one SNR (trainer.py:398-423) on `detector` as it stands.  For each of n_minibatches:
        tx, rx = words(minibatch, 'train')                                              (:400)
        j_hat = unique(randint(window_size, n_words, [meta_j_num]))                     (:404-406; or the recorded values)
        tx = rs_encode(tx, n_symbols) when n_symbols > 0                                (:407-410)
        one step per j_hat: support words j_hat + arange(-window_size, 0), query j_hat  (:413-417)
        tx, rx = words(minibatch, 'val') -> ser                                         (:420)
        the weights are saved after every minibatch                                     (:423)
    All steps of a minibatch are ONE online_trainer.maml_training call (one launch) with Adam on the kernel route; RMSprop, SGD, a CPU
    detector and use_kernel=False run them through meta.meta_train_loop on the same optimizer state, as eval_by_word does.
    j_hat: None, a sequence (per minibatch the values to use) or a callable minibatch -> values.  words, word_source, evaluate: as
    joint_train.
    encode(tx, n_symbols) -> codewords: replaces mvn.rs_encode (which runs on the device only)."""
    from .meta import meta_train_loop

    words = _word_source(words, word_source, detector, online_trainer, snr, gamma, n_symbols, subframes_in_frame)
    if n_symbols > 0 and encode is None:
        encode = rs_encode
    kernel = (online_trainer.words_kernel_route() and online_trainer.optimizer_type == "Adam") if hasattr(online_trainer, "words_kernel_route") else False
    losses, sers, weights, step_losses, counters, j_used = [], [], [], [], [], []
    for mb in range(n_minibatches):
        tx, rx = words(mb, "train")
        dev = rx.device
        if j_hat is None:
            j = torch.unique(torch.randint(low=window_size, high=tx.shape[0], size=[meta_j_num]))
        else:
            j = torch.as_tensor(np.asarray(j_hat(mb) if callable(j_hat) else j_hat[mb])).long().reshape(-1)
        j = j.to(dev)
        if n_symbols > 0:
            tx = torch.as_tensor(encode(tx, n_symbols)).to(device=dev, dtype=torch.float32)
        sup = j.reshape(-1, 1) + torch.arange(-window_size, 0, device=dev).reshape(1, -1)
        if kernel:
            sl = online_trainer.maml_training(rx, tx, sup, j, meta_lr, MAML, return_loss=True)
        else:
            sl = torch.stack([meta_train_loop(detector, meta_detector, online_trainer, rx, tx, sup[k], j[k:k + 1], meta_lr, MAML)
                              for k in range(j.numel())]).to(torch.float32)
        vtx, vrx = words(mb, "val")
        rows = torch.tensor([i for i in range(vtx.shape[0]) if i % subframes_in_frame != 0], dtype=torch.int64, device=vtx.device)
        ser, cnt = _validation(detector, vtx, vrx, snr, gamma, rows, n_symbols, evaluate)
        if hasattr(online_trainer, "check_status"):
            online_trainer.check_status()
        sl = sl.detach().cpu().numpy().astype(np.float32)
        loss_query = 0.0
        for v in sl:  # `loss_query +=` (trainer.py:416)
            loss_query += float(v)
        if verbose:
            print(f"Minibatch {mb + 1}, ser - {ser}, loss - {loss_query}")
        losses.append(loss_query)
        sers.append(ser)
        weights.append(_params_copy(detector))
        step_losses.append(sl)
        counters.append(cnt)
        j_used.append(j.cpu().numpy().astype(np.int64))
    return MetaTrainResult(np.asarray(losses), np.asarray(sers), weights, step_losses,
                           np.stack(counters) if counters else np.zeros((0, 4), np.int64), j_used)
