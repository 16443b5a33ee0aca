"""ctypes binding of libmvn_hip.so (C ABI: include/mvn.h).

There is deliberately NO CPU fallback: if the HIP library is missing or no gfx950 device is
usable, every 'val' call raises.  (The CPU oracle under oracle/ is test infrastructure and is
never imported from here.)
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVN_LIB_PATH", os.path.join(_PKG, "libmvn_hip.so"))  # override: A/B builds
ABI_VERSION = 6

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32

# the by-word block steps (mvn_{vnet,va}_byword_step[_path|_list]_f32) share their argument list segment by segment
_STEP_VNET = [_vp, _i64, _vp, _i64] + [_vp] * 6 + [ctypes.POINTER(ctypes.c_int64)]  # rx, rx_ld, tx, tx_ld, W1 .. b3, w_stride
_STEP_VA = [_vp, _i64, _vp, _i64, _vp, _i64]                                        # rx, rx_ld, tx, tx_ld, state_priors, Bp
_STEP_OUT = [_vp, _i64] * 5 + [_vp]             # dec, msg, enc, label_word, labels, each with its leading dimension; nerr
_STEP_SCALARS = [_i64, _i32, _i32, _i32, _i32]  # R, T, nsym, pilot, S
_STEP_LIST = [_i32, _vp, _i64, _vp]             # list_bytes, delta, delta_ld, choice

# name -> (restype, argtypes); mirrors include/mvn.h one to one
SIGNATURES = {
    "mvn_version": (ctypes.c_int, []),
    "mvn_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "mvn_device_info": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_char_p, ctypes.c_int]),
    "mvn_acs_block_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "mvn_acs_sweep_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "mvn_survivor_bytes": (ctypes.c_size_t, [_i64, _i32, _i32]),
    "mvn_acs_sweep_surv_f32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp]),
    "mvn_vnet_surv_workspace_bytes": (ctypes.c_size_t, [_i64, _i32, _i32]),
    "mvn_vnet_decode_surv_f32": (ctypes.c_int, [_vp, _i64] + [_vp] * 6 + [_vp, _i64, _vp, _vp, _vp, ctypes.c_size_t, _i64, _i32, _i32, _vp]),
    "mvn_va_decode_surv_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp]),
    "mvn_traceback_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "mvn_acs_sweep_kernel_name": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, ctypes.c_char_p, _i32]),
    "mvn_va_decode_kernel_name": (ctypes.c_int, [_i64, _i32, _i32, ctypes.c_char_p, _i32]),
    "mvn_vnet_decode_kernel_name": (ctypes.c_int, [_i64, _i32, _i32, _i32, ctypes.c_char_p, _i32]),
    "mvn_va_decode_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "mvn_vnet_logits_f32": (ctypes.c_int, [_vp] * 8 + [_i64, _i32, _vp]),
    "mvn_vnet_workspace_bytes": (ctypes.c_size_t, [_i64, _i32, _i32]),
    "mvn_vnet_decode_f32": (ctypes.c_int, [_vp, _i64] + [_vp] * 6 + [_vp, _i64, _vp, _vp, _vp, ctypes.c_size_t,
                                                                   _i64, _i32, _i32, _vp]),
    "mvn_vnet_decode_count_f32": (ctypes.c_int, [_vp, _i64] + [_vp] * 6 + [_vp, _i64, _i32, _vp, _vp, _vp, _i64,
                                                 _vp, ctypes.c_size_t, _i64, _i32, _i32, _vp]),
    "mvn_vnet_online_train_f32": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _i32] + [_vp] * 8 +
                                  [_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _i32, _vp]),
    "mvn_vnet_train_workspace_bytes": (ctypes.c_size_t, [_i32]),
    "mvn_vnet_online_train_ws_f32": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _i32] + [_vp] * 8 +
                                     [_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _i32, _vp,
                                      ctypes.c_size_t, _vp, _vp]),
    "mvn_vnet_train_words_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i32, _i32] + [_vp] * 8 +
                                 [_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _i32, _vp]),
    "mvn_vnet_train_words_states_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i32, _i32] + [_vp] * 8 +
                                        [_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _i32, _vp]),
    "mvn_vnet_maml_train_f32": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32] + [_vp] * 8 +
                                [_i64, ctypes.c_float, _i32] + [ctypes.c_float] * 4 + [_vp, _i32, _vp]),
    "mvn_vnet_maml_train_ws_f32": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32, _vp, _i32] + [_vp] * 8 +
                                   [_i64, ctypes.c_float, _i32] + [ctypes.c_float] * 4 + [_vp, _i32, _vp, ctypes.c_size_t, _vp, _vp]),
    "mvn_vnet_train_trials_workspace_bytes": (ctypes.c_size_t, [_i32, _i32, _i32, _i32]),
    "mvn_vnet_online_train_trials_f32": (ctypes.c_int, [_vp, _i32, _i32, _i32] + [ctypes.c_float] * 4 + [_i32, _vp, ctypes.c_size_t, _vp]),
    "mvn_vnet_maml_train_trials_f32": (ctypes.c_int, [_vp, _i32, _i32, _i32, ctypes.c_float, _i32] + [ctypes.c_float] * 4 +
                                       [_i32, _vp, ctypes.c_size_t, _vp]),
    "mvn_vnet_maml_train_states_trials_f32": (ctypes.c_int, [_vp, _i32, _i32, _i32, ctypes.c_float, _i32] + [ctypes.c_float] * 4 +
                                              [_i32, _vp]),
    "mvn_vnet_train_kernel_name": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i32, ctypes.c_size_t, ctypes.c_char_p, _i32]),
    "mvn_vnet_train_lds_bytes": (ctypes.c_size_t, [_i32, _i32]),
    "mvn_vnet_online_train_lds_bytes": (ctypes.c_size_t, [_i32]),
    "mvn_vnet_byword_step_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_max_symbols": (_i32, [_i32]),
    "mvn_vnet_byword_step_states_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_states_path_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_path_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_path_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_list_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + _STEP_LIST + [_vp]),
    "mvn_vnet_byword_step_list_max_symbols": (_i32, [_i32]),
    "mvn_vnet_byword_step_states_list_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + _STEP_LIST + [_vp]),
    "mvn_va_byword_step_list_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + _STEP_LIST + [_vp]),
    "mvn_va_byword_step_max_symbols": (_i32, [_i32]),
    "mvn_va_byword_step_list_max_symbols": (_i32, [_i32]),
    "mvn_va_byword_step_states_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_states_path_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_states_list_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + _STEP_LIST + [_vp]),
    "mvn_vnet_byword_step_256_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_256_path_f32": (ctypes.c_int, _STEP_VNET + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_256_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_va_byword_step_256_path_f32": (ctypes.c_int, _STEP_VA + _STEP_OUT + _STEP_SCALARS + [_vp]),
    "mvn_vnet_byword_step_256_max_symbols": (_i32, []),
    "mvn_va_byword_step_256_max_symbols": (_i32, []),
    "mvn_vnet_byword_step_256_segment": (_i32, []),
    "mvn_va_byword_step_256_segment": (_i32, []),
    "mvn_reload_switches": (None, []),
    "mvn_isi_awgn_transmit": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _i64, ctypes.c_double, _vp, _i64, _i64,
                                             _i32, _i32, _vp]),
    "mvn_generate_words_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, ctypes.c_double, ctypes.c_uint64, _i64, _i32, _i32, _vp]),
    "mvn_va_montecarlo_f32": (ctypes.c_int, [_vp, _i64, ctypes.c_double, ctypes.c_uint64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "mvn_vnet_montecarlo_f32": (ctypes.c_int, [_vp, _i64, ctypes.c_double, ctypes.c_uint64, _i64] + [_vp] * 6 +
                                [_vp, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _vp]),
    "mvn_rs_decode_bits_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "mvn_rs_encode_bits_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "mvn_count_errors": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp]),
    "mvn_lstm_workspace_bytes": (ctypes.c_size_t, [_i64, _i32]),
    "mvn_lstm_decode_f32": (ctypes.c_int, [_vp, _i64] + [_vp] * 10 + [_vp, _i64, _vp, _vp, ctypes.c_size_t, _i64, _i32, _vp]),
    "mvn_lstm_decode_kernel_name": (ctypes.c_int, [_i64, _i32, ctypes.c_char_p, _i32]),
    "mvn_lstm_train_workspace_bytes": (ctypes.c_size_t, [_i32]),
    "mvn_lstm_train_lds_bytes": (ctypes.c_size_t, [_i32]),
    "mvn_lstm_train_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _i32] + [_vp] * 12 +
                           [_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp, ctypes.c_size_t, _vp, _i32, _vp]),
    "mvn_lstm_train_kernel_name": (ctypes.c_int, [_i32, _i32, ctypes.c_char_p, _i32]),
    "mvn_lstm_maml_workspace_bytes": (ctypes.c_size_t, [_i32]),
    "mvn_lstm_maml_train_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _i32] + [_vp] * 12 +
                                [_i64] + [ctypes.c_float] * 5 + [_vp, _vp, ctypes.c_size_t, _vp, _i32, _vp]),
    "mvn_lstm_maml_kernel_name": (ctypes.c_int, [_i32, ctypes.c_char_p, _i32]),
    "mvn_lstm_trials_per_launch": (_i32, []),
    "mvn_lstm_train_trials_f32": (ctypes.c_int, [_vp, _i32, _i64, _i64, _i32] + [ctypes.c_float] * 4 + [_i32, _vp]),
    "mvn_lstm_maml_train_trials_f32": (ctypes.c_int, [_vp, _i32, _i64, _i64] + [ctypes.c_float] * 5 + [_i32, _vp]),
    "mvn_lstm_train_trials_kernel_name": (ctypes.c_int, [_i32, _i32, _i32, ctypes.c_char_p, _i32]),
    "mvn_lstm_decode_trials_workspace_bytes": (ctypes.c_size_t, [_i32, _i64, _i32]),
    "mvn_lstm_decode_trials_f32": (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_size_t, _i32, _i64, _i32, _vp]),
}


class LstmTrial(ctypes.Structure):
    """include/mvn.h: mvn_lstm_trial_t, one trial of mvn_lstm_train_trials_f32 / mvn_lstm_maml_train_trials_f32 (a HOST array of
    these is read by the call before it returns)."""
    _fields_ = [("y", _vp), ("bits", _vp), ("n_words", _i64), ("word_of_iter", _vp), ("idx", _vp), ("params", _vp), ("exp_avg", _vp),
                ("exp_avg_sq", _vp), ("loss_out", _vp), ("workspace", _vp), ("status", _vp), ("step0", _i64), ("n_iter", _i32),
                ("reserved", _i32)]

_lib = None


class MvnError(RuntimeError):
    """A libmvn_hip.so call returned non-zero."""


def load_variant(path: str):
    """Another build of the library (an A/B build, the tests' -DMVN_TEST_HOOKS build) with the same bindings; not cached."""
    if not os.path.exists(path):
        raise MvnError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the 'val' path.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.mvn_version() != ABI_VERSION:
        raise MvnError(f"{os.path.basename(path)} ABI {lib.mvn_version()} != expected {ABI_VERSION}")
    return lib


def load():
    """Load the HIP library; raises (never falls back) if it is absent."""
    global _lib
    if _lib is None:
        _lib = load_variant(LIB_PATH)
    return _lib


def reload_switches():
    """The library reads its MVN_* environment switches once per process; call this after changing one in-process."""
    if _lib is not None:
        _lib.mvn_reload_switches()


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mvn_strerror(rc).decode()
        if rc in (-1, -3):
            raise ValueError(f"{what}: {msg}")
        raise MvnError(f"{what}: {msg} (code {rc})")


def ptr(t):
    """Device pointer of a contiguous fp32/int64 torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream(device):
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


STEP_STATES = (4, 8, 32, 64, 128)  # the state counts of mvn_{vnet,va}_byword_step_states[_path|_list]_f32, next to the 16 of the six steps


def step_max_symbols(n_states: int) -> int:
    """The longest word the ViterbiNet running and path steps serve at n_states (mvn_vnet_byword_step_max_symbols; 0: not served)."""
    return int(load().mvn_vnet_byword_step_max_symbols(n_states))


def list_max_symbols(n_states: int) -> int:
    """The longest word the ViterbiNet list step serves at n_states (mvn_vnet_byword_step_list_max_symbols; 512 at 16 states, 0: not
    served)."""
    return int(load().mvn_vnet_byword_step_list_max_symbols(n_states))


def va_step_max_symbols(n_states: int) -> int:
    """The longest word the classical detector's running and path steps serve at n_states (mvn_va_byword_step_max_symbols; 1024 at 16
    states, 0: not served)."""
    return int(load().mvn_va_byword_step_max_symbols(n_states))


def va_list_max_symbols(n_states: int) -> int:
    """The longest word the classical detector's list step serves at n_states (mvn_va_byword_step_list_max_symbols; 512 at 16 states,
    0: not served)."""
    return int(load().mvn_va_byword_step_list_max_symbols(n_states))


def step256_max_symbols() -> int:
    """The longest word the ViterbiNet running and path steps serve at 256 states (mvn_vnet_byword_step_256_max_symbols)."""
    return int(load().mvn_vnet_byword_step_256_max_symbols())


def va_step256_max_symbols() -> int:
    """The longest word the classical detector's running and path steps serve at 256 states (mvn_va_byword_step_256_max_symbols)."""
    return int(load().mvn_va_byword_step_256_max_symbols())


def step256_segment(kind: str = "vnet") -> int:
    """The symbols of one LDS segment of the 256-state steps of `kind` ('vnet' / 'va'): a longer word goes through the LDS in pieces of
    this length (mvn_{vnet,va}_byword_step_256_segment)."""
    return int(getattr(load(), "mvn_%s_byword_step_256_segment" % kind)())


class BywordStep:
    """One of the by-word block steps of include/mvn.h, mvn_{kind}_byword_step[_path|_list]_f32 (kind 'vnet' / 'va', decision
    'running' / 'path' / 'list'), for words of T symbols with nsym parity bytes (list: list_bytes least reliable bytes): the symbol
    and the constant part of its argument list are resolved here, once, outside a caller's block loop.
    n_states other than 16: mvn_vnet_byword_step_states_f32, the ViterbiNet running step, and with states_path=True (what
    harness._block_step and trials._cohort_steps pass) mvn_vnet_byword_step_states_path_f32 for decision 'path'; with
    states_list=True (what they pass as well) mvn_vnet_byword_step_states_list_f32 for kind 'vnet', decision 'list' at the state
    counts of STEP_STATES; with states_va=True (what harness._block_step and ecc.list_decode pass) kind 'va' at those state counts
    resolves to mvn_va_byword_step_states[_path|_list]_f32; with states_256=True (what harness._block_step passes) n_states == 256
    with decision 'running' / 'path' resolves to mvn_{kind}_byword_step_256[_path]_f32; ValueError else."""
    def __init__(self, kind: str, decision: str, T: int, nsym: int, list_bytes=None, n_states: int = 16, states_path: bool = False,
                 states_list: bool = False, states_va: bool = False, states_256: bool = False):
        self.name = "mvn_%s_byword_step%s_f32" % (kind, {"running": "", "path": "_path", "list": "_list"}[decision])
        if states_256 and n_states == 256 and kind in ("vnet", "va") and decision in ("running", "path"):
            self.name = "mvn_%s_byword_step_256%s_f32" % (kind, "_path" if decision == "path" else "")
        elif states_va and kind == "va" and n_states in STEP_STATES:
            self.name = "mvn_va_byword_step_states%s_f32" % {"running": "", "path": "_path", "list": "_list"}[decision]
        elif states_list and kind == "vnet" and decision == "list" and n_states in STEP_STATES:
            self.name = "mvn_vnet_byword_step_states_list_f32"
        elif n_states != 16:
            if kind != "vnet" or decision not in (("running", "path") if states_path else ("running",)):
                raise ValueError(f"the block step at {n_states} states is the ViterbiNet running step (kind='vnet', decision='running'; "
                                 f"states_path=True: decision='path' as well), not kind={kind!r}, decision={decision!r}")
            self.name = "mvn_vnet_byword_step_states%s_f32" % ("_path" if decision == "path" else "")
        self.n_states = n_states
        self.fn = getattr(load(), self.name)
        self.no_T, self.no_K = (None, T), (None, T - 8 * nsym)  # an output that is not asked for, with its row's length
        self.T, self.nsym = T, nsym
        if (decision == "list") != (list_bytes is not None):
            raise ValueError("list_bytes belongs to decision='list', and decision='list' needs it")
        self.list_bytes = list_bytes

    def __call__(self, device, rx, rx_ld, tx, tx_ld, front, out, nerr, R, pilot, delta=None, delta_ld=None, choice=None, stream=None):
        """One launch on `device` (None: the caller holds the device guard and passes `stream`), checked.  rx / tx / nerr / delta /
        choice: pointers (ptr(); None = NULL); front: the detector's part of the list, (W1, b1, W2, b2, W3, b3, w_stride) or
        (state_priors, Bp); out: {"dec" | "msg" | "enc" | "label_word" | "labels": (pointer, leading dimension)}, what is not named is
        not written."""
        get, no_T, T = out.get, self.no_T, self.T
        tail = () if self.list_bytes is None else (self.list_bytes, delta, T if delta_ld is None else delta_ld, choice)
        with _NO_GUARD if device is None else on_device(device):
            rc = self.fn(rx, rx_ld, tx, tx_ld, *front, *get("dec", no_T), *get("msg", self.no_K), *get("enc", no_T),
                         *get("label_word", no_T), *get("labels", no_T), nerr, R, T, self.nsym, 1 if pilot else 0, self.n_states, *tail,
                         current_stream(device) if stream is None else stream)
        if rc:
            check(rc, self.name)


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_GUARD = _NoGuard()


def on_device(device):
    """`with on_device(t.device):` makes t's GPU current for a launch; free when it already is (the by-word evaluation
    issues hundreds of B=1 calls, where torch.cuda.device()'s get/set pair is a measurable part of each)."""
    import torch

    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(idx)


def f32c(t):
    """t as a contiguous fp32 tensor; the tensor itself when it already is one (only its data_ptr is used: no autograd
    bookkeeping is involved, so no detach())."""
    import torch

    if t.dtype is torch.float32 and t.is_contiguous():
        return t
    return t.detach().to(torch.float32).contiguous()


def require_gpu_tensor(t, name):
    if not t.is_cuda:
        raise MvnError(
            f"{name} lives on {t.device}: the 'val' hot path only runs on an MI355X (ROCm) device; "
            "CPU execution is intentionally not provided")
