"""CPU-only: the LSTM trial axis (meta-viterbinet_amd/lstm_trials.py; mvn_lstm_train_trials_f32, mvn_lstm_maml_train_trials_f32 and
mvn_lstm_decode_trials_f32 on the GPU).  The C ABI's argument checks without a device, the descriptor's layout against the header,
the two new kernels' resources in the gfx950 code object, LSTMTrialBank's layout and round trips, and the refusals of
eval_by_word_batched with an LSTM bank."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from meta_viterbinet_amd import lstm_trials as LT
from test_lstm_train_host import default_init_weights, detector_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvn_lstm_trials_per_launch", "mvn_lstm_train_trials_f32", "mvn_lstm_maml_train_trials_f32", "mvn_lstm_decode_trials_f32",
       "mvn_lstm_decode_trials_workspace_bytes", "mvn_lstm_train_trials_kernel_name")
FAKE = 4096  # a non-null 16-byte-aligned address that is never dereferenced: every check below happens before a device call


def trial(**kw):
    t = mvn._lib.LstmTrial()
    for f in ("y", "bits", "word_of_iter", "idx", "params", "exp_avg", "exp_avg_sq", "loss_out", "workspace", "status"):
        setattr(t, f, FAKE)
    t.n_words, t.step0, t.n_iter = 3, 0, 5
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def array(*ts):
    a = (mvn._lib.LstmTrial * len(ts))()
    for i, t in enumerate(ts):
        a[i] = t
    return a


def test_symbols_bound_and_version():
    lib = mvn._lib.load()
    raw = ctypes.CDLL(mvn._lib.LIB_PATH)
    for name in NEW:
        assert name in mvn._lib.SIGNATURES and hasattr(lib, name) and hasattr(raw, name)
    assert lib.mvn_version() == 6


@pytest.mark.parametrize("meta", [False, True])
def test_training_trials_validation(meta):
    lib = mvn._lib.load()

    def call(ts, R=None, T=136, y_ld=136, bits_ld=136, M=32):
        a = array(*ts) if ts is not None else None
        R = len(ts) if R is None else R
        p = ctypes.addressof(a) if a is not None else None
        if meta:
            return lib.mvn_lstm_maml_train_trials_f32(p, R, y_ld, bits_ld, 0.1, 1e-3, 0.9, 0.999, 1e-8, T, None)
        return lib.mvn_lstm_train_trials_f32(p, R, y_ld, bits_ld, M, 1e-3, 0.9, 0.999, 1e-8, T, None)

    ok, idle = trial(), trial(n_iter=0)
    assert call([ok], R=-1) == -1
    assert call([ok], T=0) == -1 and call([ok], T=257, y_ld=300, bits_ld=300) == -1
    assert call([ok], y_ld=135) == -1 and call([ok], bits_ld=135) == -1
    if not meta:
        assert call([ok], M=-1) == -1 and call([ok], M=137) == -1
    assert call([ok, trial(n_iter=-1)]) == -1 and call([ok, trial(n_words=0)]) == -1 and call([ok, trial(step0=-1)]) == -1
    assert call([idle, trial(n_iter=0, n_words=0)]) == -1  # an idle trial's shape is checked too
    assert call([trial(y=None)], T=0) == -1 and call([trial(y=None, n_iter=-1)]) == -1  # shapes before pointers
    assert call([], R=0) == 0 and call(None, R=0) == 0
    # idle trials are neither read nor written: no pointer of theirs is looked at
    nothing = trial(n_iter=0, y=None, bits=None, word_of_iter=None, idx=None, params=None, exp_avg=None, exp_avg_sq=None, loss_out=None,
                    workspace=None, status=None)
    assert call([nothing, nothing, idle]) == 0
    assert call(None, R=2) == -4
    for f in ("y", "bits", "params", "exp_avg", "exp_avg_sq"):
        assert call([ok, trial(**{f: None})]) == -4, f
    assert call([trial(idx=None)]) == -4  # minibatch positions (M > 0) resp. the support words
    if meta:
        assert call([trial(word_of_iter=None)]) == -4  # the query words
    else:  # whole-word iterations read no idx, word 0 needs no word_of_iter: such a call gets past the pointer checks
        assert call([trial(idx=None, workspace=None)], M=0) == -5 and call([trial(word_of_iter=None, workspace=None)]) == -5
    assert call([trial(y=None, workspace=None)]) == -4  # pointers before the workspace
    assert call([ok, trial(workspace=None)]) == -5 and call([ok, trial(workspace=FAKE + 4)]) == -5
    assert call([trial(params=FAKE + 8)]) == -5  # 16-byte loads of the matrices
    assert call([trial(loss_out=None, status=None, workspace=None)]) == -5  # loss_out and status may be NULL


def test_decode_trials_validation_and_workspace():
    lib = mvn._lib.load()
    P = 795138
    for R, B, T in ((1, 1, 136), (5, 17, 5), (8, 300, 1)):
        one = lib.mvn_lstm_workspace_bytes(B, T)
        assert lib.mvn_lstm_decode_trials_workspace_bytes(R, B, T) == R * ((one + 15) & ~15)
    assert lib.mvn_lstm_decode_trials_workspace_bytes(0, 1, 136) == 0 and lib.mvn_lstm_decode_trials_workspace_bytes(2, 0, 136) == 0
    assert lib.mvn_lstm_decode_trials_workspace_bytes(2, 1, 0) == 0
    ws = lib.mvn_lstm_decode_trials_workspace_bytes(3, 2, 136)

    def call(y=FAKE, y_ld=136, params=FAKE, param_ld=P + 2, dec=FAKE, dec_ld=136, wsp=FAKE, wsb=ws, R=3, B=2, T=136):
        return lib.mvn_lstm_decode_trials_f32(y, y_ld, params, param_ld, dec, dec_ld, None, wsp, wsb, R, B, T, None)

    assert call(R=-1) == -1 and call(B=-1) == -1 and call(T=0) == -1 and call(y_ld=135) == -1 and call(dec_ld=135) == -1
    assert call(param_ld=P) == -1 and call(param_ld=P + 1) == -1 and call(param_ld=P + 3) == -1  # below the row, or not a multiple of 4
    assert call(T=0, y=None) == -1  # shapes before pointers
    assert call(R=0, y=None, wsp=None) == 0 and call(B=0, y=None, wsp=None) == 0
    assert call(y=None) == -4 and call(params=None) == -4 and call(dec=None) == -4
    assert call(wsp=None) == -5 and call(wsb=ws - 4) == -5 and call(wsp=FAKE + 4) == -5
    buf = ctypes.create_string_buffer(128)
    assert lib.mvn_lstm_train_trials_kernel_name(4, 136, 0, buf, 128) == 0 and b"lstm_train_trials_kernel" in buf.value
    assert lib.mvn_lstm_train_trials_kernel_name(4, 136, 1, buf, 128) == 0 and b"lstm_maml_trials_kernel" in buf.value
    assert lib.mvn_lstm_train_trials_kernel_name(4, 257, 0, buf, 128) == -1 and lib.mvn_lstm_train_trials_kernel_name(-1, 136, 0, buf, 128) == -1
    assert lib.mvn_lstm_train_trials_kernel_name(4, 136, 0, None, 128) == -4
    assert 0 <= lib.mvn_lstm_trials_per_launch() <= 8


def test_trial_descriptor_layout_matches_the_header():
    """_lib.LstmTrial is include/mvn.h's mvn_lstm_trial_t field for field (compiled here with the host compiler)."""
    fields = [f for f, _ in mvn._lib.LstmTrial._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mvn.h"\nint main(void){printf("%zu", sizeof(mvn_lstm_trial_t));' + "".join(
        f'printf(" %zu", offsetof(mvn_lstm_trial_t, {f}));' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert len(fields) == 14
    assert out[0] == ctypes.sizeof(mvn._lib.LstmTrial)
    assert out[1:] == [getattr(mvn._lib.LstmTrial, f).offset for f in fields]


def test_trials_kernels_in_code_object_no_scratch():
    """lstm_train_trials_kernel and lstm_maml_trials_kernel are in the gfx950 code object, neither spills, and both take
    lstm_train_kernel's static LDS (their dynamic LDS is the same LtLds: one workgroup per CU)."""
    import __graft_entry__ as g

    so = g.build_hip()
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    bundler, readelf = os.path.join(llvm, "clang-offload-bundler"), os.path.join(llvm, "llvm-readelf")
    assert os.path.exists(bundler) and os.path.exists(readelf) and shutil.which("c++filt")
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, elf = os.path.join(tmp, "fatbin"), os.path.join(tmp, "dev.elf")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, so, os.path.join(tmp, "unused")],
                       check=True)
        subprocess.run([bundler, "--unbundle", "--type=o", "--input=" + fatbin, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--output=" + elf], check=True)
        notes = subprocess.run([readelf, "--notes", elf], check=True, capture_output=True, text=True).stdout
    table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")], input=notes, check=True,
                           capture_output=True, text=True).stdout
    rows = [re.match(r"(.+?)\s+vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) static_lds (\d+)$", ln) for ln in table.splitlines()]
    rows = {m.group(1): m for m in rows if m}
    for name in ("lstm_train_kernel", "lstm_train_trials_kernel", "lstm_maml_trials_kernel"):
        assert name in rows, name
        print(f"{name}: {rows[name].group(2)} VGPRs, {rows[name].group(3)} SGPRs, scratch {rows[name].group(4)}, static LDS {rows[name].group(5)}")
    one = rows["lstm_train_kernel"]
    for name in ("lstm_train_trials_kernel", "lstm_maml_trials_kernel"):
        assert int(rows[name].group(4)) == 0
        assert int(rows[name].group(5)) == int(one.group(5))
    assert int(one.group(5)) + mvn._lib.load().mvn_lstm_train_lds_bytes(256) <= 160 * 1024
    assert 2 * (int(one.group(5)) + mvn._lib.load().mvn_lstm_train_lds_bytes(1)) > 160 * 1024  # a CU holds ONE such workgroup, at every T


@pytest.fixture(scope="module")
def two_sets():
    return [default_init_weights(3), default_init_weights(4)]


def test_bank_layout_views_and_round_trip(two_sets):
    bank = mvn.LSTMTrialBank(two_sets, "cpu", lr=2e-3, optimizer_type="RMSprop", train_minibatch_size=8)
    assert bank.R == 2 and bank.optimizer_type == "RMSprop" and bank.train_minibatch_size == 8 and bank.lr == 2e-3
    assert LT.N_PARAMS == 795138 and LT.ROW == 795140 and LT.ROW % 4 == 0
    for t in (bank.theta, bank.saved, bank.exp_avg, bank.exp_avg_sq):
        assert tuple(t.shape) == (2, 795140) and t.stride(0) % 4 == 0 and t.is_contiguous() and t.dtype is torch.float32
    assert bank.step.dtype == np.int64 and bank.step.shape == (2,) and not bank.step.any()
    assert bank.status.dtype is torch.int32 and bank.status.numel() == 2
    assert not bank.exp_avg.any() and not bank.exp_avg_sq.any() and torch.equal(bank.theta, bank.saved)
    assert bank.kernel_optimizer_args() == (-1.0, 0.99, 1e-8)
    for r in range(2):
        for saved in (False, True):
            views = bank.weights(r, saved)
            assert [tuple(v.shape) for v in views] == mvn.lstm.PARAM_SHAPES
            assert all(np.array_equal(v.numpy(), w) for v, w in zip(views, two_sets[r]))
            base = (bank.saved if saved else bank.theta)
            at = base.data_ptr() + 4 * 795140 * r
            for v in views:  # views of the bank, back to back in parameters() order
                assert v.data_ptr() == at
                at += 4 * v.numel()
    bank.weights(1)[8][1, 5] = 7.5  # fc weight [2, 256]
    assert float(bank.theta[1, 794624 + 256 + 5]) == 7.5 and float(bank.saved[1, 794624 + 256 + 5]) != 7.5
    # the round trip with an LSTMDetector's state_dict
    det = bank.load_into(mvn.LSTMDetector().to("cpu"), 1)
    assert list(det.state_dict().keys())[0].startswith("lstm.") and list(det.state_dict().keys())[-1] == "fc.bias"
    assert all(torch.equal(p.detach(), v) for p, v in zip(det._params(), bank.weights(1)))
    assert float(det.fc.weight.detach()[1, 5]) == 7.5
    det0 = detector_with(two_sets[0])
    bank.store_from(det0, 1)
    bank.store_from(det, 0, saved=True)
    assert torch.equal(bank.theta[1], bank.theta[0]) and float(bank.saved[0, 794624 + 256 + 5]) == 7.5
    assert all(np.array_equal(v.numpy(), w) for v, w in zip(bank.weights(1), two_sets[0]))
    back = bank.load_into(mvn.LSTMDetector().to("cpu"), 0, saved=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), det.state_dict().values()))
    assert not bank.theta[:, 795138:].any()  # the padding stays zero


def test_bank_refusals(two_sets):
    with pytest.raises(NotImplementedError, match="optimizer"):
        mvn.LSTMTrialBank(two_sets, "cpu", optimizer_type="Adagrad")
    with pytest.raises(ValueError, match="ten arrays"):
        mvn.LSTMTrialBank([two_sets[0][:6]], "cpu")
    with pytest.raises(ValueError, match="parameter count"):
        mvn.LSTMTrialBank([two_sets[0][:9] + [np.zeros(3, np.float32)]], "cpu")
    bank = mvn.LSTMTrialBank(two_sets[:1], "cpu")
    assert not isinstance(bank, mvn.TrialBank)
    bank.check_status()  # nothing outstanding
    with pytest.raises(mvn._lib.MvnError, match=r"trials \[1\]"):
        bank.check_status(np.array([0, 1]))


def test_eval_by_word_batched_refusals_before_any_device(two_sets):
    bank = mvn.LSTMTrialBank(two_sets, "cpu")
    tx, rx = torch.zeros(2, 3, 120), torch.zeros(2, 3, 136)
    draws = [mvn.TrialDraws(1, "cpu"), mvn.TrialDraws(2, "cpu")]
    kw = dict(n_symbols=2, subframes_in_frame=25)
    with pytest.raises(ValueError, match="harness.eval_by_word"):
        mvn.eval_by_word_batched(bank, tx, rx, draws=draws, online_meta=True, MAML=False, weights_init="random", **kw)
    with pytest.raises(ValueError, match="weights init"):
        mvn.eval_by_word_batched(bank, tx, rx, draws=draws, weights_init="nonsense", **kw)
    with pytest.raises(ValueError, match="meta_training_weights"):
        mvn.eval_by_word_batched(bank, tx, rx, draws=draws, online_meta=True, MAML=False, weights_init="meta_training", **kw)
    with pytest.raises(ValueError, match="one bank row per trial"):
        mvn.eval_by_word_batched(bank, tx[:1], rx[:1], draws=draws[:1], **kw)
    with pytest.raises(ValueError, match="one bank row per trial"):
        mvn.eval_by_word_batched(bank, tx, rx, draws=draws[:1], **kw)
    with pytest.raises(ValueError, match="one bank row per trial"):
        mvn.eval_by_word_batched(bank, tx[:, :, :100], rx, draws=draws, **kw)
    assert LT.lock_step_serves(136, True, False, 1) and LT.lock_step_serves(256, False, True, 3)
    assert not LT.lock_step_serves(136, True, True, 1) and not LT.lock_step_serves(136, True, False, 2) and not LT.lock_step_serves(257, False, False, 1)
