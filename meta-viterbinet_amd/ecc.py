"""Reed-Solomon outer code on the GPU: counterpart of python_code/ecc/rs_main.py (encode :9-18, decode :21-37),
batched over words so the detect -> RS-decode -> count loop of trainer.py:232-239 / :295-305 never leaves the device."""
import math

import numpy as np
import torch

from . import _lib


def _bits(t: torch.Tensor) -> torch.Tensor:
    _lib.require_gpu_tensor(t, "bits")
    if t.dtype is not torch.float32:
        t = t.detach().to(torch.float32)
    if t.dim() == 1:
        t = t.reshape(1, -1)
    return t if t.stride(-1) == 1 else t.contiguous()


def rs_decode(detected_words: torch.Tensor, n_symbols: int, return_status: bool = False):
    """[B, K + 8*n_symbols] detected bits -> [B, K] decoded message bits (fp32 {0.,1.}), like
    `[decode(w, n_symbols) for w in detected_words]` in trainer.py:235."""
    rx = _bits(detected_words)
    B, N = rx.shape
    if N % 8 or N // 8 <= n_symbols:
        raise ValueError("word length must be a multiple of 8 bits and longer than the parity")
    if N // 8 > 255:
        raise ValueError("Message is too long (%i when max is 255)" % (N // 8))
    out = torch.empty((B, N - 8 * n_symbols), dtype=torch.float32, device=rx.device)
    status = torch.empty(B, dtype=torch.int32, device=rx.device) if return_status else None
    with _lib.on_device(rx.device):
        rc = _lib.load().mvn_rs_decode_bits_f32(_lib.ptr(rx), rx.stride(0), _lib.ptr(out), out.stride(0), _lib.ptr(status), B,
                                                N, n_symbols, _lib.current_stream(rx.device))
    _lib.check(rc, "mvn_rs_decode_bits_f32")
    return (out, status) if return_status else out


def rs_encode(words: torch.Tensor, n_symbols: int) -> torch.Tensor:
    """[B, K] message bits -> [B, K + 8*n_symbols] systematic codewords (rs_main.py:9-18, trainer.py:304)."""
    msg = _bits(words)
    B, K = msg.shape
    if K % 8:
        raise ValueError("word length must be a multiple of 8 bits")
    if K // 8 + n_symbols > 255:
        raise ValueError("Message is too long (%i when max is 255)" % (K // 8 + n_symbols))
    out = torch.empty((B, K + 8 * n_symbols), dtype=torch.float32, device=msg.device)
    with _lib.on_device(msg.device):
        rc = _lib.load().mvn_rs_encode_bits_f32(_lib.ptr(msg), msg.stride(0), _lib.ptr(out), out.stride(0), B, K, n_symbols,
                                                _lib.current_stream(msg.device))
    _lib.check(rc, "mvn_rs_encode_bits_f32")
    return out


LIST_MAX_T = 512         # the list step keeps branch costs and forward metrics in LDS (include/mvn.h)
LIST_MAX_CANDIDATES = 63  # one erasure pattern per lane of a wavefront, next to the hard decoder's word


def list_bytes_for(T: int, n_symbols: int, list_bytes=None) -> int:
    """The number m of least reliable bytes a list decode draws its erasures from: list_bytes, or n_symbols + 2 capped by the
    word's bytes.  ValueError when m is outside n_symbols <= m <= T / 8 or C(m, n_symbols) exceeds 63 candidates."""
    n = T // 8
    m = min(n_symbols + 2, n) if list_bytes is None else int(list_bytes)
    if not n_symbols <= m <= n:
        raise ValueError(f"list_bytes must lie in [n_symbols, T / 8] = [{n_symbols}, {n}], got {m}")
    if math.comb(m, n_symbols) > LIST_MAX_CANDIDATES:
        raise ValueError(f"list_bytes = {m} gives C({m}, {n_symbols}) = {math.comb(m, n_symbols)} erasure patterns; "
                         f"at most {LIST_MAX_CANDIDATES} are evaluated")
    return m


def list_step_bytes(T: int, n_symbols: int, list_bytes=None, what: str = "decision='list'") -> int:
    """The shapes the list step serves, checked in one place for eval_by_word, eval_by_word_batched and list_decode: words of whole
    bytes longer than the parity, 1 <= n_symbols <= 8, T <= 512; returns the validated list_bytes (list_bytes_for).  ValueError
    names the condition that does not hold."""
    if not (T % 8 == 0 and 1 <= n_symbols <= 8 and T // 8 > n_symbols):
        raise ValueError(f"{what} needs words of whole bytes longer than the parity and 1 <= n_symbols <= 8 (T = {T}, n_symbols = {n_symbols})")
    if T > LIST_MAX_T:
        raise ValueError(f"{what} serves words of up to {LIST_MAX_T} symbols (branch costs and forward metrics stay in LDS), got T = {T}")
    return list_bytes_for(T, n_symbols, list_bytes)


def list_decode(detector, rx: torch.Tensor, n_symbols: int, list_bytes=None, return_delta: bool = False, gamma: float = None,
                count: int = None):
    """Reliability-ordered list decoding of B received words in ONE launch (mvn_vnet_byword_step_list_f32 /
    mvn_va_byword_step_list_f32 without a transmitted word): every word is detected along its traced-back Viterbi path, its
    max-log LLRs delta rank the bytes, n_symbols of the list_bytes (default n_symbols + 2) least reliable bytes are erased in every
    combination and filled, and of those codewords and the hard-decoded one the one whose own path through the detector's branch
    costs is cheapest wins (include/mvn.h has the exact arithmetic).
    detector: a 16-state VNETDetector or VADetector (gamma / count: what VADetector.forward takes to find the words' channel), or a
    VNETDetector at 4, 8, 32, 64 or 128 states (mvn_vnet_byword_step_states_list_f32, T <= _lib.list_max_symbols(n_states)), or a
    VADetector at those state counts (mvn_va_byword_step_states_list_f32, T <= _lib.va_list_max_symbols(n_states));
    rx [B, T], T a multiple of 8 and <= 512.  Returns (msg [B, T - 8 n_symbols] fp32 bits, choice [B] int32: 0 = the hard decoder's
    word, c > 0 = the c-th erasure pattern) and, with return_delta, delta [B, T]."""
    from .detectors import VADetector, VNETDetector

    if not isinstance(detector, (VADetector, VNETDetector)):
        raise ValueError(f"list_decode needs a Viterbi / ViterbiNet detector, not {type(detector).__name__}")
    T = rx.shape[-1]
    S = getattr(detector, "n_states", None)
    states = S in _lib.STEP_STATES  # mvn_vnet_byword_step_states_list_f32 / mvn_va_byword_step_states_list_f32
    if S != 16 and not states:
        raise ValueError("list_decode runs the 16-state kernels, and the ViterbiNet and Viterbi kernels at 4, 8, 32, 64 and 128 states")
    m = list_step_bytes(T, n_symbols, list_bytes, "list_decode")
    if states:
        longest = _lib.va_list_max_symbols(S) if isinstance(detector, VADetector) else _lib.list_max_symbols(S)
        if T > longest:
            raise ValueError(f"list_decode serves words of up to {longest} symbols at {S} states, got T = {T}")
    if isinstance(detector, VADetector) and gamma is None:
        raise ValueError("list_decode with a VADetector needs gamma (what VADetector.forward takes to find the words' channel)")
    y = _bits(rx)
    B, K = y.shape[0], T - 8 * n_symbols
    dev = y.device
    msg = torch.empty((B, K), dtype=torch.float32, device=dev)
    choice = torch.empty(B, dtype=torch.int32, device=dev)
    delta = torch.empty((B, T), dtype=torch.float32, device=dev) if return_delta else None
    if isinstance(detector, VADetector):
        if detector.transmission_length != T:
            raise ValueError(f"the detector's transmission_length {detector.transmission_length} is not the word length {T}")
        pri = detector._priors_table(y, gamma, "val", count)
        if B % pri.shape[0] != 0:
            raise ValueError(f"{B} words do not divide into the detector's {pri.shape[0]} rows of state priors")
        kind, front = "va", (_lib.ptr(pri), pri.shape[0])
    else:
        if detector.transmission_lengths["val"] != T:
            raise ValueError(f"the detector's 'val' length {detector.transmission_lengths['val']} is not the word length {T}")
        kind, front = "vnet", (*[_lib.ptr(_lib.f32c(p)) for p in detector._params()], None)
    _lib.BywordStep(kind, "list", T, n_symbols, m, n_states=S, states_list=True, states_va=True)(dev, _lib.ptr(y), y.stride(0), None, K, front, {"msg": (_lib.ptr(msg), K)}, None, B,
                                                   False, delta=_lib.ptr(delta), choice=_lib.ptr(choice))
    return (msg, choice, delta) if return_delta else (msg, choice)


def encode(binary_word: np.ndarray, nsym: int) -> np.ndarray:
    """Single-word NumPy signature of the reference (rs_main.py:9)."""
    dev = torch.device("cuda")
    return rs_encode(torch.as_tensor(np.asarray(binary_word), dtype=torch.float32, device=dev), nsym)[0].cpu().numpy().astype(int)


def decode(binary_rx: np.ndarray, nsym: int) -> np.ndarray:
    """Single-word NumPy signature of the reference (rs_main.py:21)."""
    dev = torch.device("cuda")
    return rs_decode(torch.as_tensor(np.asarray(binary_rx), dtype=torch.float32, device=dev), nsym)[0].cpu().numpy().astype(int)
