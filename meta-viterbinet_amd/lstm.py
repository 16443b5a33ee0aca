"""LSTM detectors: same constructors, forward() signatures, constants and state_dict keys as
python_code/detectors/LSTM/lstm_detector.py and detectors/META_LSTM/meta_lstm_detector.py.  Phase 'val' runs on the MI355X through
libmvn_hip.so (mvn_lstm_decode_f32: window, both layers, fc and argmax in one kernel); every other phase returns the logits from
torch autograd.  LSTM online training and meta-learning are not built: the harness's update branches refuse these detectors."""
import torch
import torch.nn as nn
from torch.nn import functional as F

from . import _lib

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
