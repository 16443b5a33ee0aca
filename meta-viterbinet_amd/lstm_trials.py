"""R LSTM detectors on ONE GPU: the trial axis of the three LSTM curves (LSTM, OnlineRNN, Meta-LSTM).

One trial's training launch is 64 workgroups, a quarter of an MI355X, and its iteration a latency-bound chain of device-wide
exchanges; mvn_lstm_train_trials_f32 / mvn_lstm_maml_train_trials_f32 run P = mvn_lstm_trials_per_launch() trials side by side in
one launch (csrc/lstm_train.inc), mvn_lstm_decode_trials_f32 detects the R words of a block step in one launch (csrc/lstm.inc).
LSTMTrialBank holds the R detectors and their optimizer state in stacked device tensors; eval_by_word (reached through
trials.eval_by_word_batched) steps R by-word evaluations through their blocks together.  Per trial every result -- decisions,
weights, moments, losses -- is bit for bit that of the single-trial calls on the trial alone (tests/test_gpu_lstm_trials.py)."""
import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .lstm import N_CLASSES, PARAM_SHAPES, TRAIN_MAX_T, LSTMDetector, LSTMMetaTrainer
from .metrics import ser_from_errors

N_PARAMS = sum(int(np.prod(s)) for s in PARAM_SHAPES)  # 795138
# A bank row: 795138 is 2 mod 4 and the training kernels read the matrices with 16-byte loads, so the stride is padded to a multiple of 4
ROW = (N_PARAMS + 3) & ~3
_OFF = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in PARAM_SHAPES])]).astype(np.int64)


def _flat_row(w) -> torch.Tensor:
    return torch.cat([torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach().cpu(), dtype=torch.float32).reshape(-1)
                      for a in w])


class LSTMTrialBank:
    """Weights, saved weights (the reference's saved_detector, trainer.py:275) and optimizer state of R LSTM detectors in stacked
    device tensors [R, ROW]; row r is trial r, a row holds the ten arrays flat in parameters() order (lstm.PARAM_SHAPES) and two
    floats of padding.  step: int64 [R] on the host.  One status word and one training workspace per trial."""

    def __init__(self, weights: Sequence[Sequence], device, lr: float = 0.001, betas=(0.9, 0.999), eps: float = 1e-8,
                 optimizer_type: str = "Adam", train_minibatch_size: int = 32):
        if optimizer_type not in ("Adam", "RMSprop", "SGD"):  # deep_learning_setup (trainer.py:163-175)
            raise NotImplementedError("No such optimizer implemented!!!")
        self.optimizer_type = optimizer_type
        self.R = len(weights)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.train_minibatch_size = train_minibatch_size
        self.device = torch.device(device)
        self.P = N_PARAMS
        rows = []
        for w in weights:
            if len(w) != len(PARAM_SHAPES):
                raise ValueError("a trial's weights are ten arrays in parameters() order")
            row = _flat_row(w)
            if row.numel() != self.P:
                raise ValueError(f"LSTM parameter count {row.numel()} != {self.P}")
            rows.append(torch.cat([row, torch.zeros(ROW - self.P)]))
        self.theta = (torch.stack(rows) if rows else torch.zeros((0, ROW))).to(self.device).contiguous()
        self.saved = self.theta.clone()
        self.exp_avg = torch.zeros_like(self.theta)
        self.exp_avg_sq = torch.zeros_like(self.theta)
        self.step = np.zeros(self.R, dtype=np.int64)
        self.status = torch.zeros(max(self.R, 1), dtype=torch.int32, device=self.device)
        self._ws = None
        self._unchecked = False

    def weights(self, r: int, saved: bool = False) -> List[torch.Tensor]:
        """Trial r's ten arrays as views with the shapes of LSTMDetector's parameters()."""
        row = (self.saved if saved else self.theta)[r]
        return [row[int(_OFF[a]):int(_OFF[a + 1])].reshape(s) for a, s in enumerate(PARAM_SHAPES)]

    def load_into(self, detector: LSTMDetector, r: int, saved: bool = False) -> LSTMDetector:
        """Trial r's weights into an LSTMDetector (through its state_dict, in parameters() order)."""
        sd = detector.state_dict()
        names = [n for n, _ in detector.lstm.named_parameters(prefix="lstm")] + [n for n, _ in detector.fc.named_parameters(prefix="fc")]
        for n, w in zip(names, self.weights(r, saved)):
            sd[n] = w.detach().clone().to(sd[n].device)
        detector.load_state_dict(sd)
        return detector

    def store_from(self, detector: LSTMDetector, r: int, saved: bool = False):
        """An LSTMDetector's weights into row r (theta, or the saved weights)."""
        row = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in detector._params()])
        if row.numel() != self.P:
            raise ValueError(f"LSTM parameter count {row.numel()} != {self.P}")
        (self.saved if saved else self.theta)[r, :self.P].copy_(row)

    def kernel_optimizer_args(self):
        """(beta1, beta2, eps) as the training kernels take them (OnlineTrainer.kernel_optimizer_args)."""
        if self.optimizer_type == "RMSprop":
            return -1.0, 0.99, 1e-8
        if self.optimizer_type == "SGD":
            return -2.0, 0.0, 0.0
        return self.betas[0], self.betas[1], self.eps

    def workspaces(self, T: int) -> torch.Tensor:
        """uint8 [R, bytes]: one meta-learning workspace (which holds the training workspace) per trial."""
        need = (int(_lib.load().mvn_lstm_maml_workspace_bytes(T)) + 255) & ~255
        if need == 0:
            raise ValueError(f"words of length {T}: the training kernels take 1 <= T <= {TRAIN_MAX_T}")
        if self._ws is None or self._ws.shape[1] < need:
            self._ws = torch.empty((max(self.R, 1), need), dtype=torch.uint8, device=self.device)
        return self._ws

    def _descriptors(self, trials, y, bits, n_words, word_of_iter, idx, n_iter, loss_out, T):
        ws = self.workspaces(T)
        d = (_lib.LstmTrial * len(trials))()
        for k, r in enumerate(trials):
            d[k].y, d[k].bits, d[k].n_words = y[k], bits[k], int(n_words[k])
            d[k].word_of_iter = word_of_iter[k] if word_of_iter is not None else None
            d[k].idx = idx[k] if idx is not None else None
            d[k].params = self.theta.data_ptr() + 4 * ROW * r
            d[k].exp_avg = self.exp_avg.data_ptr() + 4 * ROW * r
            d[k].exp_avg_sq = self.exp_avg_sq.data_ptr() + 4 * ROW * r
            d[k].loss_out = loss_out[k] if loss_out is not None else None
            d[k].workspace = ws.data_ptr() + ws.stride(0) * r
            d[k].status = self.status.data_ptr() + 4 * r
            d[k].step0, d[k].n_iter, d[k].reserved = int(self.step[r]), int(n_iter[k]), 0
        return d

    def train_trials(self, trials: Sequence[int], y, bits, n_words, n_iter, T: int, M: int = 0, idx=None, word_of_iter=None,
                     loss_out=None, y_ld: Optional[int] = None, bits_ld: Optional[int] = None):
        """n_iter[k] iterations of mvn_lstm_train_f32 for trial trials[k], all trials in one mvn_lstm_train_trials_f32 call.
        y[k], bits[k] (and idx[k], word_of_iter[k], loss_out[k]): DEVICE ADDRESSES (ints) of the trial's words [n_words[k], T]
        (fp32 / int32, row strides y_ld / bits_ld, default T), minibatch positions int32 [n_iter[k], M], word numbers int32
        [n_iter[k]] and loss vector; the caller keeps those tensors alive until the stream has run the call."""
        if len(trials) == 0:
            return
        d = self._descriptors(trials, y, bits, n_words, word_of_iter, idx if M > 0 else None, n_iter, loss_out, T)
        b1, b2, eps = self.kernel_optimizer_args()
        with _lib.on_device(self.device):
            rc = _lib.load().mvn_lstm_train_trials_f32(ctypes.addressof(d), len(trials), y_ld or T, bits_ld or T, M, self.lr, b1, b2, eps, T,
                                                       _lib.current_stream(self.device))
        _lib.check(rc, "mvn_lstm_train_trials_f32")
        self._unchecked = True
        for k, r in enumerate(trials):
            self.step[r] += int(n_iter[k])

    def maml_trials(self, trials: Sequence[int], y, bits, n_words, support_idx, query_idx, n_steps, T: int, meta_lr: float,
                    loss_out=None, y_ld: Optional[int] = None, bits_ld: Optional[int] = None):
        """n_steps[k] first-order meta-learning steps of mvn_lstm_maml_train_f32 for trial trials[k] in one
        mvn_lstm_maml_train_trials_f32 call; support_idx[k], query_idx[k]: device addresses of int32 [n_steps[k]]."""
        if len(trials) == 0:
            return
        d = self._descriptors(trials, y, bits, n_words, query_idx, support_idx, n_steps, loss_out, T)
        b1, b2, eps = self.kernel_optimizer_args()
        with _lib.on_device(self.device):
            rc = _lib.load().mvn_lstm_maml_train_trials_f32(ctypes.addressof(d), len(trials), y_ld or T, bits_ld or T, meta_lr, self.lr, b1,
                                                            b2, eps, T, _lib.current_stream(self.device))
        _lib.check(rc, "mvn_lstm_maml_train_trials_f32")
        self._unchecked = True
        for k, r in enumerate(trials):
            self.step[r] += int(n_steps[k])

    def check_status(self, values=None):
        """Raises MvnError naming the trials whose training launch abandoned its device-wide barrier (their weights are NaN).
        values: the R status words when the caller has just read them; otherwise one R-word device-to-host copy, and only when a
        launch is outstanding."""
        if not self._unchecked and values is None:
            return
        self._unchecked = False
        st = np.asarray(self.status[:self.R].cpu() if values is None else values)
        if st.any():
            self.status.zero_()
            raise _lib.MvnError(f"LSTM trials {np.flatnonzero(st).tolist()}: {_lib.load().mvn_strerror(-7).decode()}")


def lstm_decode_trials(y: torch.Tensor, bank: LSTMTrialBank, return_logits: bool = False):
    """y [R, B, T] -> decisions [R, B, T] fp32 {0,1} (and the logits [R, B, T, 2]): trial r's B words detected with bank row r,
    all R x B words in one launch of mvn_lstm_decode_trials_f32.  y may be row-strided (unit stride along T, the trials B rows
    apart); trial r's output is bit for bit lstm_decode(y[r], bank.weights(r))."""
    _lib.require_gpu_tensor(y, "y")
    if y.dim() != 3 or y.shape[0] != bank.R:
        raise ValueError(f"y must be [R = {bank.R}, B, T], got {tuple(y.shape)}")
    R, B, T = y.shape
    # the call has ONE row stride for the R B rows: a trial's rows y_ld apart and the trials B y_ld apart (B = 1: any trial stride)
    if y.dtype is torch.float32 and y.stride(2) == 1 and B == 1 and (y.stride(0) >= T or R == 1):
        yc, y_ld = y, max(y.stride(0), T)
    elif y.dtype is torch.float32 and y.stride(2) == 1 and y.stride(1) >= T and (y.stride(0) == B * y.stride(1) or R == 1):
        yc, y_ld = y, y.stride(1)
    else:
        yc, y_ld = _lib.f32c(y), T
    lib = _lib.load()
    dec = torch.empty((R, B, T), dtype=torch.float32, device=yc.device)
    logits = torch.empty((R, B, T, N_CLASSES), dtype=torch.float32, device=yc.device) if return_logits else None
    ws_bytes = int(lib.mvn_lstm_decode_trials_workspace_bytes(R, B, T))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=yc.device)  # the R weight sets in the kernel's fragment order
    with _lib.on_device(yc.device):
        rc = lib.mvn_lstm_decode_trials_f32(_lib.ptr(yc), y_ld, _lib.ptr(bank.theta), ROW, _lib.ptr(dec), T, _lib.ptr(logits),
                                            _lib.ptr(ws), ws_bytes, R, B, T, _lib.current_stream(yc.device))
    _lib.check(rc, "mvn_lstm_decode_trials_f32")
    return (dec, logits) if return_logits else dec


def lock_step_serves(T: int, online_meta: bool, MAML: bool, window_size: int) -> bool:
    """Does the lock-step engine run such an evaluation (otherwise: trial after trial through harness.eval_by_word)?"""
    return 1 <= T <= TRAIN_MAX_T and not (online_meta and (MAML or window_size != 1))


def eval_by_word(bank: LSTMTrialBank, tx, rx, n_symbols, subframes_in_frame, draws, self_supervised, self_supervised_iterations,
                 ser_thresh, online_meta, meta_lr, MAML, window_size, meta_train_iterations, meta_j_num, meta_subframes,
                 meta_style_online_training, weights_init, meta_training_weights, record, initial_buffer) -> np.ndarray:
    """trials.eval_by_word_batched for an LSTMTrialBank (it has checked R and prepared `record` and `initial_buffer` [R, W0, T]);
    see its docstring.  One block step, for all R trials together: one detection launch; RS decode, error count and re-encoding
    of the R words; one transfer of the R error counts and status words and one host sync; the reference's per-trial decisions
    (harness.py, the update branches of eval_by_word) on the host; at most one meta-learning launch for the trials whose update
    is due and at most one training launch for the trials with ser <= ser_thresh."""
    from .ecc import rs_decode, rs_encode

    R, N, T = rx.shape
    K = tx.shape[2]
    if weights_init == "random":
        raise ValueError("weights_init='random' re-initialises an LSTM detector from torch's global generator (LSTMDetector()'s own "
                         "draws), so a trial cannot be replayed on its own: run harness.eval_by_word trial by trial")
    if weights_init == "meta_training" and meta_training_weights is None:
        raise ValueError("weights_init='meta_training' needs meta_training_weights (ten arrays in parameters() order)")
    if tx.shape[1] != N or K != T - 8 * n_symbols:
        raise ValueError("tx [R, N, K], rx [R, N, K + 8 n_symbols], one TrialDraws and one bank row per trial")
    ser_by_word = np.zeros((R, N))
    if R == 0 or N == 0:
        return ser_by_word
    if not lock_step_serves(T, online_meta, MAML, window_size):
        return _one_trial_at_a_time(bank, tx, rx, n_symbols, subframes_in_frame, draws, ser_by_word, record, initial_buffer,
                                    dict(self_supervised=self_supervised, self_supervised_iterations=self_supervised_iterations,
                                         ser_thresh=ser_thresh, online_meta=online_meta, meta_lr=meta_lr, MAML=MAML, window_size=window_size,
                                         meta_train_iterations=meta_train_iterations, meta_j_num=meta_j_num, meta_subframes=meta_subframes,
                                         meta_style_online_training=meta_style_online_training, weights_init=weights_init,
                                         meta_training_weights=meta_training_weights))
    _lib.require_gpu_tensor(rx, "rx")
    dev = rx.device
    rx = _lib.f32c(rx)
    tx = _lib.f32c(tx).to(dev)
    full_word = meta_style_online_training
    M = 0 if full_word else bank.train_minibatch_size
    # A trial's words: the W0 words its buffer starts with (buffer_empty=False), then its N blocks; word number = position here
    W0 = 0 if initial_buffer is None else int(initial_buffer[0].shape[1])
    NA = W0 + N
    labels = torch.zeros((R, NA, T), dtype=torch.int32, device=dev)  # the bits a buffered word is trained on
    if W0:
        rx = torch.cat([initial_buffer[1].to(dev), rx], dim=1).contiguous()
        labels[:, :W0] = initial_buffer[0].to(dev).to(torch.int32)
    sync_dev = torch.zeros(2 * R, dtype=torch.int32, device=dev)  # [0:R] bit errors of the step, [R:2R] the status words
    sync_host = torch.zeros(2 * R, dtype=torch.int32).pin_memory()
    nerr_np, status_np = sync_host.numpy()[:R], sync_host.numpy()[R:]
    rx_p = [rx.data_ptr() + 4 * NA * T * r for r in range(R)]
    lab_p = [labels.data_ptr() + 4 * NA * T * r for r in range(R)]
    max_steps = meta_train_iterations * meta_j_num
    idx_host = torch.zeros((R, 2, max(max_steps, 1)), dtype=torch.int32).pin_memory() if online_meta else None
    idx_dev = torch.zeros((R, 2, max(max_steps, 1)), dtype=torch.int32, device=dev) if online_meta else None
    init_row = None
    if weights_init == "meta_training":
        init_row = torch.cat([_flat_row(meta_training_weights), torch.zeros(ROW - N_PARAMS)]).to(dev)
        if init_row.numel() != ROW:
            raise ValueError(f"LSTM parameter count {init_row.numel() - (ROW - N_PARAMS)} != {N_PARAMS}")
    if online_meta or meta_style_online_training:
        bank.saved.copy_(bank.theta)  # saved_detector = copy.deepcopy(detector) (trainer.py:275)
    buffers: List[List[int]] = [list(range(W0)) for _ in range(R)]  # trial r's buffer: the word numbers it holds, oldest first
    held = None

    def rows(which):
        return torch.as_tensor(np.asarray(which, dtype=np.int64), device=dev)

    with _lib.on_device(dev):
        for count in range(N):
            pilot = count % subframes_in_frame == 0
            at = W0 + count
            if pilot:  # the word is known (trainer.py:314-316); its detection feeds nothing
                labels[:, at] = rs_encode(tx[:, count], n_symbols).to(torch.int32)
                sync_dev[:R].zero_()
            else:
                detected = lstm_decode_trials(rx[:, at:at + 1], bank).reshape(R, T)
                decoded = rs_decode(detected, n_symbols)
                nerr = (decoded != tx[:, count]).sum(dim=1, dtype=torch.int32)
                sync_dev[:R] = nerr
                # the word the reference buffers: the detected word if ser > 0, else the re-encoded one (ser > 0 <=> an error)
                labels[:, at] = torch.where(nerr[:, None] > 0, detected, rs_encode(decoded, n_symbols)).to(torch.int32)
            sync_dev[R:] = bank.status[:R]
            sync_host.copy_(sync_dev, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()  # the one host sync of the step
            bank.check_status(status_np)
            ser = np.zeros(R) if pilot else ser_from_errors(nerr_np, K)  # the reference's value bit for bit (metrics.py:13-16)
            if not pilot:
                ser_by_word[:, count] = ser
            if record is not None:
                record["nerr"][:, count] = nerr_np
            push = ser <= ser_thresh  # trainer.py:319-324
            for r in np.flatnonzero(push):
                buffers[r].append(at)
                if W0:  # buffer_empty=False: a window of fixed length, the oldest word leaves (:325-328)
                    del buffers[r][0]
            # ---- online meta-learning (trainer.py:331-343): restart from the saved weights, all steps of all due trials in one launch
            if online_meta and count % meta_subframes == 0 and count >= meta_subframes:
                act = [r for r in range(R) if len(buffers[r]) > 2]
                if act:
                    ns = []
                    for r in act:
                        buf = np.asarray(buffers[r], dtype=np.int32)
                        j_hat = draws[r].j_hat_update(len(buf) - 2, meta_train_iterations, meta_j_num)
                        n = j_hat.shape[0]
                        idx_host[r, 0, :n] = torch.from_numpy(buf[(j_hat - 1) % len(buf)])  # support: the word before, from the end for 0
                        idx_host[r, 1, :n] = torch.from_numpy(buf[j_hat])                   # query
                        ns.append(n)
                        if record is not None:
                            record["meta"][r, count] = True
                    idx_dev.copy_(idx_host, non_blocking=True)  # (rewritten only after the next step's sync, which follows the copy)
                    a = rows(act)
                    bank.theta[a] = bank.saved[a] if weights_init == "last_frame" else init_row.expand(len(act), ROW)
                    stride = idx_dev.stride(0) * 4
                    bank.maml_trials(act, [rx_p[r] for r in act], [lab_p[r] for r in act], [NA] * len(act),
                                     [idx_dev.data_ptr() + stride * r for r in act],
                                     [idx_dev.data_ptr() + stride * r + 4 * idx_dev.stride(1) for r in act], ns, T, meta_lr)
                    bank.saved[a] = bank.theta[a]
            # ---- self-supervised training on the word just buffered (trainer.py:345-347)
            if self_supervised and push.any():
                act = [int(r) for r in np.flatnonzero(push)]
                # this block's minibatches from each trial's own draws (a TrialDraws hands out a view of its device table); `held`
                # keeps them alive until the stream has run the launch, i.e. past the next step's sync
                held = [draws[r].batches(count, N, T, self_supervised_iterations, M).to(device=dev, dtype=torch.int32).contiguous()
                        for r in act] if M else None
                if meta_style_online_training:  # metavnet_trainer.py:59
                    a = rows(act)
                    bank.theta[a] = bank.saved[a]
                idx = [t.data_ptr() for t in held] if M else None
                bank.train_trials(act, [rx_p[r] + 4 * at * T for r in act], [lab_p[r] + 4 * at * T for r in act], [1] * len(act),
                                  [self_supervised_iterations] * len(act), T, M, idx)
                if record is not None:
                    record["trained"][act, count] = True
        bank.check_status()
    return ser_by_word


def _one_trial_at_a_time(bank, tx, rx, n_symbols, subframes_in_frame, draws, ser_by_word, record, initial_buffer, kw):
    """The evaluations the lock-step engine does not serve -- second-order meta-learning, a window of several support words, words
    longer than the training kernels take -- one trial after the other through harness.eval_by_word with an LSTMMetaTrainer on a
    detector loaded from the bank; weights, saved weights, optimizer state and step counts go back into the bank."""
    from .harness import eval_by_word as eval_one

    for r in range(bank.R):
        det = bank.load_into(LSTMDetector().to(bank.device), r)
        tr = LSTMMetaTrainer(det, lr=bank.lr, betas=bank.betas, eps=bank.eps, train_minibatch_size=bank.train_minibatch_size,
                             optimizer_type=bank.optimizer_type)
        tr.exp_avg.copy_(bank.exp_avg[r, :bank.P])
        tr.exp_avg_sq.copy_(bank.exp_avg_sq[r, :bank.P])
        tr.step = int(bank.step[r])
        last = {}

        def observer(seen, last=last):
            last.update(seen)
            if record is not None and seen["stage"] == "end":
                record["trained"][r, seen["count"]] = seen["trained"]
                record["meta"][r, seen["count"]] = seen["meta"] is not None

        ser_by_word[r] = eval_one(det, tx[r], rx[r], 0.0, 0.0, n_symbols, subframes_in_frame, online_trainer=tr, draws=draws[r],
                                  initial_buffer=None if initial_buffer is None else (initial_buffer[0][r], initial_buffer[1][r]),
                                  observer=observer, **kw)
        bank.store_from(det, r)
        saved = last.get("saved_detector")
        bank.store_from(saved if saved is not None else det, r, saved=True)
        bank.exp_avg[r, :bank.P].copy_(tr.exp_avg)
        bank.exp_avg_sq[r, :bank.P].copy_(tr.exp_avg_sq)
        bank.step[r] = tr.step
    return ser_by_word
