"""One launcher for the six by-word block steps through the raw ctypes symbols (mvn_{vnet,va}_byword_step[_path|_list]_f32), shared by
test_gpu_byword_codec.py, test_gpu_path_step.py and test_gpu_list_step.py.  It marshals the argument list itself -- not through
mvn._lib.BywordStep, which is code under test."""
import ctypes

import numpy as np
import torch

import meta_viterbinet_amd as mvn

SENTINEL = {"dec": 7.0, "msg": 7.0, "enc": 7.0, "lw": 7.0, "labels": -1, "nerr": -1, "delta": 7.0, "choice": -1}
OUTPUTS = ("dec", "msg", "enc", "lw", "labels", "nerr")  # of every variant; 'list' adds delta and choice
INT = ("labels", "nerr", "choice")
SUFFIX = {"running": "_f32", "path": "_path_f32", "list": "_list_f32"}


def padded(a, ld, fill, dev):
    """Rows of `a` at leading dimension ld on the device, the padding filled with `fill`."""
    a = np.asarray(a, np.float32)
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return torch.as_tensor(out).to(dev)


def step(dev, variant, kind, rx, tx, nsym, pilot=False, m=None, want=None, ld=None, pri=None, Bp=1, weights=None, w_stride=None):
    """One launch of variant 'running' / 'path' / 'list' (m = list_bytes) of the VA step (kind 'va': pri [Bp, 16] on the device, None:
    NULL) or the ViterbiNet step (kind 'vnet': weights = six device tensors or pointers, w_stride = None or six strides).  rx [R, T] /
    tx [R, K] are host arrays (None: NULL; rx None takes R and T from tx); ld: leading dimensions by name (rx, tx and the outputs;
    default: the row length), the padding of rx filled with NaN and that of tx with 7.  Outputs not in `want` (default: all the
    variant has) are passed as NULL.  Returns the requested outputs as host arrays INCLUDING their padding, pre-filled with SENTINEL,
    and the row lengths."""
    R = tx.shape[0] if rx is None else rx.shape[0]
    T = tx.shape[1] + 8 * nsym if rx is None else rx.shape[1]
    K = T - 8 * nsym
    row = {"rx": T, "tx": K, "dec": T, "msg": K, "enc": T, "lw": T, "labels": T, "delta": T}
    lds = dict(row, **(ld or {}))
    rx_d = None if rx is None else padded(rx, lds["rx"], np.nan, dev)
    tx_d = None if tx is None else padded(tx, lds["tx"], 7.0, dev)
    has = OUTPUTS + (("delta", "choice") if variant == "list" else ())
    want = has if want is None else tuple(n for n in want if n in has)
    out = {}
    for name in want:
        shape = (R,) if name in ("nerr", "choice") else (R, lds[name])
        out[name] = torch.full(shape, SENTINEL[name], dtype=torch.int32 if name in INT else torch.float32, device=dev)
    p = lambda name: mvn._lib.ptr(out.get(name))  # noqa: E731
    tail = (p("dec"), lds["dec"], p("msg"), lds["msg"], p("enc"), lds["enc"], p("lw"), lds["lw"], p("labels"), lds["labels"], p("nerr"),
            R, T, nsym, 1 if pilot else 0, 16)
    if variant == "list":
        tail += (m, p("delta"), lds["delta"], p("choice"))
    tail += (mvn._lib.current_stream(dev),)
    if kind == "va":
        front = (mvn._lib.ptr(pri), Bp)
    else:
        front = (*[a if isinstance(a, ctypes.c_void_p) else mvn._lib.ptr(a) for a in weights],
                 None if w_stride is None else (ctypes.c_int64 * 6)(*w_stride))
    rc = getattr(mvn._lib.load(), f"mvn_{kind}_byword_step{SUFFIX[variant]}")(mvn._lib.ptr(rx_d), lds["rx"], mvn._lib.ptr(tx_d), lds["tx"],
                                                                              *front, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize(dev)
    return {name: t.cpu().numpy() for name, t in out.items()}, row
