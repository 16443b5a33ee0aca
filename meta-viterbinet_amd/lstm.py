"""LSTM detectors: same constructors, forward() signatures, constants and state_dict keys as
python_code/detectors/LSTM/lstm_detector.py and detectors/META_LSTM/meta_lstm_detector.py.  Phase 'val' runs on the MI355X through
libmvn_hip.so (mvn_lstm_decode_f32: window, both layers, fc and argmax in one kernel); every other phase returns the logits from
torch autograd.  LSTMOnlineTrainer trains an LSTMDetector -- online on one word (lstm_trainer.py:42-53, meta_lstm_trainer.py:48-60)
or jointly, one word per step (trainer.py:470-479) -- with every iteration of a call inside one launch of mvn_lstm_train_f32
(forward, CrossEntropy, backward through time and the optimizer step; csrc/lstm_train.inc).  LSTMMetaTrainer adds the online
meta-learning of MetaLSTMTrainer (Trainer.meta_train_loop, trainer.py:425-453): first order with one support word per step in one
launch of mvn_lstm_maml_train_f32, second order and longer windows through MetaLSTMDetector on torch autograd."""
import torch
import torch.nn as nn
from torch.nn import functional as F

from . import _lib
from .online import OnlineTrainer

INPUT_SIZE = 4  # lstm_detector.py:6-10
HIDDEN_SIZE = 256
NUM_LAYERS = 2
N_CLASSES = 2
START_VALUE_PADDING = -100

_G = 4 * HIDDEN_SIZE
# nn.LSTM.parameters() order (per layer W_ih, W_hh, b_ih, b_hh), then fc weight, bias
PARAM_SHAPES = [(_G, INPUT_SIZE), (_G, HIDDEN_SIZE), (_G,), (_G,), (_G, HIDDEN_SIZE), (_G, HIDDEN_SIZE), (_G,), (_G,),
                (N_CLASSES, HIDDEN_SIZE), (N_CLASSES,)]


def _default_device():
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def sliding_windows(y: torch.Tensor) -> torch.Tensor:
    """[B, T] -> [B, T, INPUT_SIZE]: x_t = (y[t-3], y[t-2], y[t-1], y[t]), START_VALUE_PADDING where the index is negative -- what the
    reference's right padding and rolls build (lstm_detector.py:42-44)."""
    padded = F.pad(y, [INPUT_SIZE - 1, 0], value=START_VALUE_PADDING)
    return padded.unfold(1, INPUT_SIZE, 1).contiguous()


def _weights_on(params, device):
    w = [_lib.f32c(p) if p.device == device else _lib.f32c(p).to(device) for p in params]
    if len(w) != len(PARAM_SHAPES) or any(tuple(t.shape) != s for t, s in zip(w, PARAM_SHAPES)):
        raise ValueError(f"LSTM parameter shapes {[tuple(t.shape) for t in w]} != {PARAM_SHAPES}")
    return w


def lstm_decode(y: torch.Tensor, params, return_logits: bool = False):
    """The 'val' path of both detectors -> mvn_lstm_decode_f32: decisions [B, T] fp32 {0,1} (and the logits [B, T, 2]).
    params: the ten arrays in PARAM_SHAPES order, read at call time.  A row-strided y (unit column stride) is read in place."""
    _lib.require_gpu_tensor(y, "y")
    if y.dim() != 2:
        raise ValueError(f"y must be [B, T], got {tuple(y.shape)}")
    yc = y if (y.dtype is torch.float32 and y.stride(1) == 1 and y.stride(0) >= y.shape[1]) else _lib.f32c(y)
    B, T = yc.shape
    w = _weights_on(params, yc.device)
    lib = _lib.load()
    dec = torch.empty((B, T), dtype=torch.float32, device=yc.device)
    logits = torch.empty((B, T, N_CLASSES), dtype=torch.float32, device=yc.device) if return_logits else None
    ws_bytes = int(lib.mvn_lstm_workspace_bytes(B, T))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=yc.device)  # the weights in the kernel's fragment order
    with _lib.on_device(yc.device):
        rc = lib.mvn_lstm_decode_f32(_lib.ptr(yc), max(yc.stride(0), T), *[_lib.ptr(t) for t in w], _lib.ptr(dec), T, _lib.ptr(logits),
                                     _lib.ptr(ws), ws_bytes, B, T, _lib.current_stream(yc.device))
    _lib.check(rc, "mvn_lstm_decode_f32")
    return (dec, logits) if return_logits else dec


class LSTMDetector(nn.Module):
    """The windowed two-layer LSTM detector (lstm_detector.py:14-59); parameter names lstm.* and fc.* match the reference so
    checkpoints interchange."""

    def __init__(self):
        super().__init__()
        self.lstm = nn.LSTM(INPUT_SIZE, HIDDEN_SIZE, NUM_LAYERS, batch_first=True, bidirectional=False).to(_default_device())
        self.fc = nn.Linear(HIDDEN_SIZE, N_CLASSES).to(_default_device())

    def _params(self):
        return list(self.lstm.parameters()) + list(self.fc.parameters())

    def forward(self, y: torch.Tensor, phase: str, snr: float = None, gamma: float = None, count: int = None) -> torch.Tensor:
        """'val' -> detected words [B, T] fp32 {0,1} (the kernel); otherwise the logits [B, T, 2] with autograd.  The reference calls
        nn.LSTM once per word (:48-50); the words are independent, so one batched call is the same function."""
        if phase == "val":
            return lstm_decode(y, self._params())
        B, T = y.shape[0], y.shape[1]
        out, _ = self.lstm(sliding_windows(y))  # zero initial h and c (:38-39)
        return self.fc(out.reshape(-1, HIDDEN_SIZE)).reshape(B, T, N_CLASSES)


class MetaLSTMDetector(nn.Module):
    """The same network with its weights passed as `var` (meta_lstm_detector.py:15-72: ten arrays in LSTMDetector's parameters()
    order), the cell unrolled with F.linear so that MAML can differentiate through an inner step.  Owns no parameters."""

    def __init__(self):
        super().__init__()

    def forward(self, y: torch.Tensor, phase: str, var: list) -> torch.Tensor:
        if phase == "val":
            return lstm_decode(y, list(var))
        B, T = y.shape[0], y.shape[1]
        x = sliding_windows(y)
        h = [y.new_zeros(B, HIDDEN_SIZE) for _ in range(NUM_LAYERS)]
        c = [y.new_zeros(B, HIDDEN_SIZE) for _ in range(NUM_LAYERS)]
        top = []
        for t in range(T):
            inp = x[:, t]
            for layer in range(NUM_LAYERS):
                w_ih, w_hh, b_ih, b_hh = var[4 * layer: 4 * layer + 4]
                gates = F.linear(inp, w_ih, b_ih) + F.linear(h[layer], w_hh, b_hh)
                i, f, g, o = gates.chunk(4, dim=1)
                c[layer] = torch.sigmoid(f) * c[layer] + torch.sigmoid(i) * torch.tanh(g)
                h[layer] = torch.sigmoid(o) * torch.tanh(c[layer])
                inp = h[layer]
            top.append(inp)
        out = torch.stack(top, dim=1).reshape(-1, HIDDEN_SIZE)
        return F.linear(out, var[-2], var[-1]).reshape(B, T, N_CLASSES)


TRAIN_MAX_T = 256  # MVN_LSTM_TRAIN_MAX_T (include/mvn.h): longer words take the autograd route


class LSTMOnlineTrainer(OnlineTrainer):
    """The optimizer state (exp_avg, exp_avg_sq, step) of an LSTMDetector's ten parameters, like the optimizer
    deep_learning_setup() creates (trainer.py:163-175), and the training loops of LSTMTrainer / MetaLSTMTrainer on it.  Same duck
    type as OnlineTrainer (params, exp_avg, exp_avg_sq, step, sync_words / status / check_status, reset_state, select_batches,
    kernel_optimizer_args, optimizer_type, use_kernel).  use_kernel=True (the default) runs mvn_lstm_train_f32; use_kernel=False, a CPU detector or a word longer than TRAIN_MAX_T takes stock autograd on the same
    state: the cross-check of the kernel and the CPU route."""

    def __init__(self, detector, lr: float = 0.001, betas=(0.9, 0.999), eps: float = 1e-8, train_minibatch_size: int = 32,
                 use_kernel: bool = True, optimizer_type: str = "Adam"):
        # use_kernel=True is the default because the kernel route is the faster one (profiles/lstm_train_time.txt: 1.10 ms against
        # 14.8 ms per iteration at T = 136)
        if optimizer_type not in ("Adam", "RMSprop", "SGD"):  # deep_learning_setup (trainer.py:163-175)
            raise NotImplementedError("No such optimizer implemented!!!")
        if not isinstance(detector, LSTMDetector):
            raise ValueError("LSTMOnlineTrainer trains an LSTMDetector")
        self.detector = detector
        self.optimizer_type = optimizer_type
        self.use_kernel = use_kernel
        self.memory_length = None
        self.lr, self.betas, self.eps = lr, betas, eps
        self.train_minibatch_size = train_minibatch_size
        self.params = detector._params()
        if [tuple(p.shape) for p in self.params] != PARAM_SHAPES:
            raise ValueError(f"LSTM parameter shapes {[tuple(p.shape) for p in self.params]} != {PARAM_SHAPES}")
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step = 0
        self.sync_words = torch.zeros(2, dtype=torch.int32, device=dev) if dev.type == "cuda" else None
        self.status = self.sync_words[1:2] if dev.type == "cuda" else None
        self._unchecked = False

    def maml_training(self, *args, **kwargs):
        raise NotImplementedError("LSTMOnlineTrainer does not meta-learn: use LSTMMetaTrainer(detector)")

    def kernel_route(self, T: int) -> bool:
        """Does a call on words of length T run mvn_lstm_train_f32?"""
        return bool(self.use_kernel and self.params[0].is_cuda and 1 <= T <= TRAIN_MAX_T)

    def _workspace(self, T: int, dev) -> torch.Tensor:
        ws = getattr(self, "_ws", None)
        need = int(_lib.load().mvn_lstm_train_workspace_bytes(T))
        if ws is None or ws.device != dev or ws.numel() < need:
            ws = self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def online_training(self, tx: torch.Tensor, rx: torch.Tensor, iterations: int = 200, batch_idx: torch.Tensor = None,
                        full_word: bool = False, return_loss: bool = False, labels: torch.Tensor = None):
        """`iterations` steps on ONE word: tx [1, T] its bits (the labels), rx [1, T] the received word.  full_word=False is
        LSTMTrainer's form (lstm_trainer.py:30-53: the loss over train_minibatch_size positions per iteration, batch_idx
        [iterations, M] or drawn by select_batches); full_word=True MetaLSTMTrainer's (meta_lstm_trainer.py:38-60: the whole word).
        labels is accepted for OnlineTrainer's signature and unused (the labels are tx)."""
        T = rx.reshape(-1).numel()
        idx = None
        if not full_word:
            idx = self.select_batches(T, iterations) if batch_idx is None else batch_idx
            if idx.dim() != 2 or idx.shape[0] != iterations:
                raise ValueError("batch_idx must be [iterations, M]")
        return self._train(tx.reshape(1, T), rx.reshape(1, T), None, iterations, idx, return_loss)

    def train_words(self, tx_words: torch.Tensor, rx_words: torch.Tensor, batch_idx: torch.Tensor = None, full_word: bool = False,
                    return_loss: bool = False):
        """One step per row of tx_words / rx_words [n, T], in row order: the inner loop of Trainer.train() (trainer.py:476-479)."""
        n, T = rx_words.shape
        idx = None
        if not full_word:
            idx = self.select_batches(T, n) if batch_idx is None else batch_idx
            if idx.dim() != 2 or idx.shape[0] != n:
                raise ValueError("batch_idx must be [n_words, M]")
        return self._train(tx_words, rx_words, torch.arange(n, dtype=torch.int32), n, idx, return_loss)

    def _train(self, tx, rx, word_of_iter, iterations, idx, return_loss):
        p = self.params
        dev = p[0].device
        T = rx.shape[1]
        if not self.kernel_route(T):
            return self._train_autograd(tx, rx, word_of_iter, iterations, idx, return_loss)
        _lib.require_gpu_tensor(rx, "rx")
        y = _lib.f32c(rx)
        bits = tx.detach().to(device=dev, dtype=torch.int32).contiguous()
        M = 0
        if idx is not None:
            idx = idx.to(device=dev, dtype=torch.int32).contiguous()
            M = idx.shape[1]
        woi = None if word_of_iter is None else word_of_iter.to(device=dev, dtype=torch.int32).contiguous()
        for t in p:
            if not t.data.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("LSTM parameters must be contiguous fp32")
        loss = torch.empty(iterations, dtype=torch.float32, device=dev) if return_loss else None
        ws = self._workspace(T, dev)
        b1, b2, eps = self.kernel_optimizer_args()
        with _lib.on_device(dev):
            rc = _lib.load().mvn_lstm_train_f32(_lib.ptr(y), T, _lib.ptr(bits), T, y.shape[0], _lib.ptr(woi), _lib.ptr(idx), M, iterations,
                                                *[_lib.ptr(t.data) for t in p], _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                                self.step, self.lr, b1, b2, eps, _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                                _lib.ptr(self.status), T, _lib.current_stream(dev))
        _lib.check(rc, "mvn_lstm_train_f32")
        self._unchecked = True
        self.step += iterations
        return loss

    def _train_autograd(self, tx, rx, word_of_iter, iterations, idx, return_loss):
        """The same loop on stock PyTorch autograd (run_train_loop, trainer.py:492-505): LSTMDetector(rx, 'train'), CrossEntropy
        over the selected positions, optimizer_step on the shared exp_avg / exp_avg_sq / step."""
        p = self.params
        dev = p[0].device
        y = rx.detach().to(device=dev, dtype=p[0].dtype)
        lab = tx.detach().to(dev).long()
        if idx is not None:
            idx = idx.to(dev).long()
        losses = []
        for it in range(iterations):
            w = 0 if word_of_iter is None else int(word_of_iter[it])
            logits = self.detector(y[w:w + 1], "train").reshape(-1, N_CLASSES)
            loss = F.cross_entropy(logits, lab[w]) if idx is None else F.cross_entropy(logits[idx[it]], lab[w][idx[it]])
            self.optimizer_step(torch.autograd.grad(loss, p))
            if return_loss:
                losses.append(loss.detach())
        return torch.stack(losses).to(torch.float32) if return_loss else None


class LSTMMetaTrainer(LSTMOnlineTrainer):
    """LSTMOnlineTrainer plus the online meta-learning of the Meta-LSTM curve: Trainer.meta_train_loop (trainer.py:425-453) as
    MetaLSTMTrainer runs it from eval_by_word (:331-343), on the same optimizer state as online_training.  First-order steps
    (MAML=False) with one support word run on the GPU, every step of a call inside one launch of mvn_lstm_maml_train_f32
    (csrc/lstm_train.inc); second order, several support words, a CPU detector, a word longer than TRAIN_MAX_T and
    use_kernel=False take torch autograd through MetaLSTMDetector on the same state (meta_kernel_route says which)."""

    # use_kernel=True stays the default for the first-order route: 2.18 ms against 220 ms per step at T = 136
    # (profiles/lstm_meta_time.txt)
    def meta_kernel_route(self, T: int, W: int = 1, MAML: bool = False) -> bool:
        """Does a maml_training call on words of length T with W support words per step run mvn_lstm_maml_train_f32?"""
        return bool(self.kernel_route(T) and W == 1 and not MAML)

    def maml_training(self, rx_words: torch.Tensor, tx_words: torch.Tensor, support_idx: torch.Tensor, query_idx: torch.Tensor,
                      meta_lr: float, MAML: bool = True, return_loss: bool = False, labels: torch.Tensor = None):
        """n meta-learning steps, OnlineTrainer.maml_training's semantics: rx_words / tx_words [Nw, T] the buffered received words
        and their bits (the labels); support_idx [n, W], query_idx [n] the words of every step (negative indices count from the
        end).  Uses and advances the same optimizer state as online_training.  Returns the query losses [n] if return_loss.
        labels is accepted for OnlineTrainer's signature and unused (the labels are tx_words)."""
        p = self.params
        dev = p[0].device
        Nw, T = rx_words.shape
        qry = torch.remainder(query_idx.to(dev).reshape(-1).long(), Nw)
        n = qry.numel()
        sup = torch.remainder(support_idx.to(dev).reshape(n, -1).long(), Nw)
        W = sup.shape[1]
        if not self.meta_kernel_route(T, W, MAML):
            return self._maml_autograd(rx_words, tx_words, sup, qry, meta_lr, MAML, return_loss)
        _lib.require_gpu_tensor(rx_words, "rx_words")
        y = _lib.f32c(rx_words)
        bits = tx_words.detach().to(device=dev, dtype=torch.int32).contiguous()
        sup32, qry32 = sup.reshape(-1).to(torch.int32).contiguous(), qry.to(torch.int32).contiguous()
        for t in p:
            if not t.data.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("LSTM parameters must be contiguous fp32")
        loss = torch.empty(n, dtype=torch.float32, device=dev) if return_loss else None
        ws = self._meta_workspace(T, dev)
        b1, b2, eps = self.kernel_optimizer_args()
        with _lib.on_device(dev):
            rc = _lib.load().mvn_lstm_maml_train_f32(_lib.ptr(y), T, _lib.ptr(bits), T, Nw, _lib.ptr(sup32), _lib.ptr(qry32), n,
                                                     *[_lib.ptr(t.data) for t in p], _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                                     self.step, meta_lr, self.lr, b1, b2, eps, _lib.ptr(loss), _lib.ptr(ws), ws.numel(),
                                                     _lib.ptr(self.status), T, _lib.current_stream(dev))
        _lib.check(rc, "mvn_lstm_maml_train_f32")
        self._unchecked = True
        self.step += n
        return loss

    def _meta_workspace(self, T: int, dev) -> torch.Tensor:
        """The training workspace with the fast-weight image behind it (3.7 MB at T = 256); online_training shares it."""
        ws = getattr(self, "_ws", None)
        need = int(_lib.load().mvn_lstm_maml_workspace_bytes(T))
        if ws is None or ws.device != dev or ws.numel() < need:
            ws = self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def _maml_autograd(self, rx, tx, sup, qry, meta_lr, MAML, return_loss):
        """meta.meta_train_loop with MetaLSTMTrainer's loss (meta_lstm_trainer.py:38-46: CrossEntropy over reshape(-1, 2) against
        the bits), step after step on stock autograd; 'train' of MetaLSTMDetector differentiates twice."""
        p = self.params
        dev = p[0].device
        y = rx.detach().to(device=dev, dtype=p[0].dtype)
        lab = tx.detach().to(dev).long()
        meta_detector = MetaLSTMDetector()
        losses = []
        for k in range(qry.numel()):
            s, q = sup[k], qry[k:k + 1]
            loss_supp = F.cross_entropy(meta_detector(y[s], "train", p).reshape(-1, N_CLASSES), lab[s].reshape(-1))
            local_grad = torch.autograd.grad(loss_supp, p, create_graph=MAML)
            updated = [w - meta_lr * g for g, w in zip(local_grad, p)]
            loss_query = F.cross_entropy(meta_detector(y[q], "train", updated).reshape(-1, N_CLASSES), lab[q].reshape(-1))
            self.optimizer_step(torch.autograd.grad(loss_query, p, create_graph=False))
            if return_loss:
                losses.append(loss_query.detach())
        return torch.stack(losses).to(torch.float32) if return_loss else None
