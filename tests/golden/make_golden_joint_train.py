#!/usr/bin/env python3
"""G22 generator (the two offline loops of the ViterbiNet trainers): imports the UNMODIFIED reference on CPU, like
make_golden_lstm_train.py, and writes tests/golden/g22_joint_training.npz:

    MVN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_joint_train.py

Sizes of every flow: memory 4 (16 states), use_ecc with n_symbols 2, block 120 (words of 136 symbols), train_frames 1 x
subframes_in_frame 25 = 25 training words per minibatch, train_minibatch_num 3, val_frames 2 (50 validation words, 48 of them data),
10 dB, gamma 0.2, the static time_decay channel.

  a_{adam,rmsprop,sgd}_*  VNETTrainer.train() (trainer.py:455-490): idx [3, 25, 32] the torch.multinomial draws of select_batch
       (positions in [0, 120): calc_loss gets the 120 message bits), loss [3, 25] every run_train_loop loss, ser [3], errors [3]
       the bit errors over the data rows of each validation, best the 0-based minibatch of the last save_weights call (the strict
       ser < best_ser), lr, and the weight digests final_* and, where best is not the last minibatch, best_*
  b_{maml,fo}_*           METAVNETTrainer.meta_train() (trainer.py:383-423), window_size 1, meta_j_num 4, MAML True / False, Adam:
       randint [3, 4] the raw torch.randint draws (j_hat = their sorted unique values), loss [3, 4] the meta_train_loop query losses
       in j_hat order (NaN beyond the minibatch's steps), ser, errors, lr, meta_lr, and final_* the digest of the weights saved
       after the last minibatch (save_weights runs after every minibatch)
  shared by all flows (the datasets' two RandomState streams give every flow the same words in the same order): w0_{k} the initial
  weights, train_tx [3, 25, 120], train_rx [3, 25, 136], val_tx [3, 50, 120], val_rx [3, 50, 136], meta = [noise_seed, word_seed,
  n_symbols, subframes_in_frame, snr, memory_length]

A weight digest (prefix_p{k}, float32): the five small tensors whole; of W2 [50, 100] the 512 entries at
numpy.random.RandomState(2200).choice(5000, 512, replace=False) (p2) and the L2 norm (n2).

Condition on the fixture (no tolerance): every flow is rerun under torch.set_default_dtype(torch.float64) with the initial weights,
the words and every draw replayed, and the noise seed is the first of SEEDS for which ALL flows give the same per-minibatch error
counts and the same best minibatch in float32 and float64.  The script prints the seed it took.
"""
import contextlib
import io
import os
import sys
import tempfile

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
REF = os.environ.get("MVN_REFERENCE")  # (or the reference checkout on PYTHONPATH)
if REF and REF not in sys.path:
    sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TMP = tempfile.mkdtemp(prefix="mvn_golden_joint_train_")

import python_code.trainers.trainer as trainer_module  # noqa: E402
from python_code.channel.channel_dataset import ChannelModelDataset  # noqa: E402
from python_code.trainers.META_VNET.metavnet_trainer import METAVNETTrainer  # noqa: E402
from python_code.trainers.VNET.vnet_trainer import VNETTrainer  # noqa: E402

SEEDS = (3450002, 3450003, 3450004, 3450005, 3450006, 3450007, 3450008, 3450009)
WORD_SEED = 7860002
BASE = dict(use_ecc=True, n_symbols=2, memory_length=4, channel_type="ISI_AWGN", val_block_length=120, val_frames=2,
            subframes_in_frame=25, train_block_length=120, train_frames=1, train_minibatch_num=3, train_minibatch_size=32,
            channel_coefficients="time_decay", fading_in_channel=False, fading_in_decoder=False, fading_taps_type=1, noisy_est_var=0,
            train_SNR_start=10, train_SNR_end=10, train_SNR_step=1, val_SNR_start=10, val_SNR_end=10, val_SNR_step=1, gamma=0.2,
            loss_type="CrossEntropy", self_supervised=False, online_meta=False, eval_mode="aggregated", word_seed=WORD_SEED,
            window_size=1, meta_j_num=4, meta_lr=0.1)
# learning rates that move the weights within 75 (part a) and at most 12 (part b) steps
FLOWS = (("a_adam", VNETTrainer, dict(optimizer_type="Adam", lr=5e-3)),
         ("a_rmsprop", VNETTrainer, dict(optimizer_type="RMSprop", lr=2e-3)),
         ("a_sgd", VNETTrainer, dict(optimizer_type="SGD", lr=0.2)),
         ("b_maml", METAVNETTrainer, dict(optimizer_type="Adam", lr=5e-3, MAML=True)),
         ("b_fo", METAVNETTrainer, dict(optimizer_type="Adam", lr=5e-3, MAML=False)))
W2_POS = np.random.RandomState(2200).choice(5000, 512, replace=False)


def digest(weights, prefix, out):
    for k, w in enumerate(weights):
        w = np.asarray(w, np.float64).reshape(-1)
        if k == 2:
            out[f"{prefix}_p2"] = w[W2_POS].astype(np.float32)
            out[f"{prefix}_n2"] = np.array(np.linalg.norm(w))
        else:
            out[f"{prefix}_p{k}"] = w.astype(np.float32)


def snapshot(det):
    return [p.detach().double().numpy().copy() for p in det.parameters()]


def run_flow(cls, kw, noise_seed, replay=None):
    """One train() of `cls`; replay: a record of an earlier run whose initial weights, words and draws are played back.
    Returns the record."""
    wdir = os.path.join(TMP, f"w_{cls.__name__}_{noise_seed}_{len(os.listdir(TMP))}")
    os.makedirs(wdir, exist_ok=True)
    torch.manual_seed(2201)
    tr = cls(**dict(BASE, **kw), noise_seed=noise_seed, weights_dir=wdir)
    rec = dict(w0=None, words={"train": [], "val": []}, multinomial=[], randint=[], loss=[], meta_loss=[], ser=[], errors=[], saves=[],
               saved_weights=[])
    calls = {"train": 0, "val": 0}
    real = dict(multinomial=torch.multinomial, randint=torch.randint, getitem=ChannelModelDataset.__getitem__,
                rates=trainer_module.calculate_error_rates, init=tr.initialize_detector, loop=tr.run_train_loop,
                meta_loop=tr.meta_train_loop, save=tr.save_weights)

    def init_spy():
        real["init"]()
        if replay is not None:
            with torch.no_grad():
                for p, w in zip(tr.detector.parameters(), replay["w0"]):
                    p.copy_(torch.from_numpy(w).to(p.dtype))
        rec["w0"] = snapshot(tr.detector)

    def multinomial_spy(weights, n, *a, **k):
        r = real["multinomial"](weights, n, *a, **k)
        if replay is not None:
            r = torch.from_numpy(replay["multinomial"][len(rec["multinomial"])].astype(np.int64))
        rec["multinomial"].append(r.numpy().copy())
        return r

    def randint_spy(*a, **k):
        r = real["randint"](*a, **k)
        if replay is not None:
            r = torch.from_numpy(replay["randint"][len(rec["randint"])].astype(np.int64))
        rec["randint"].append(r.numpy().copy())
        return r

    def getitem_spy(self_, snr_list, gamma):
        b, y = real["getitem"](self_, snr_list=snr_list, gamma=gamma)
        if replay is not None:  # the float32 words of the recorded run, in this run's default dtype
            rb, ry = replay["words"][self_.phase][calls[self_.phase]]
            b, y = torch.Tensor(rb.astype(np.float64)), torch.Tensor(ry.astype(np.float64))
        calls[self_.phase] += 1
        rec["words"][self_.phase].append((b.numpy().astype(np.uint8), y.numpy().astype(np.float32)))
        return b, y

    def rates_spy(prediction, target):
        rec["errors"].append(int((prediction.long() != target.long()).sum().item()))
        res = real["rates"](prediction, target)
        rec["ser"].append(float(res[0]))
        return res

    def loop_spy(soft_estimation, transmitted_words):
        v = real["loop"](soft_estimation=soft_estimation, transmitted_words=transmitted_words)
        rec["loss"].append(float(v))
        return v

    def meta_loop_spy(received_words, transmitted_words, support_idx, query_idx):
        v = real["meta_loop"](received_words, transmitted_words, support_idx, query_idx)
        rec["meta_loss"].append((len(rec["ser"]), float(v.detach())))  # (minibatch = validations so far)
        return v

    def save_spy(current_loss, snr, gamma):
        rec["saves"].append(len(rec["ser"]) - 1)  # the minibatch whose validation has just run
        rec["saved_weights"].append(snapshot(tr.detector))
        return real["save"](current_loss, snr, gamma)

    torch.multinomial, torch.randint = multinomial_spy, randint_spy
    ChannelModelDataset.__getitem__ = getitem_spy
    trainer_module.calculate_error_rates = rates_spy
    tr.initialize_detector, tr.run_train_loop, tr.meta_train_loop, tr.save_weights = init_spy, loop_spy, meta_loop_spy, save_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train()
    finally:
        torch.multinomial, torch.randint = real["multinomial"], real["randint"]
        ChannelModelDataset.__getitem__ = real["getitem"]
        trainer_module.calculate_error_rates = real["rates"]
    rec["final"] = snapshot(tr.detector)
    return rec


def both_dtypes(cls, kw, seed):
    rec = run_flow(cls, kw, seed)
    torch.set_default_dtype(torch.float64)
    try:
        rec64 = run_flow(cls, kw, seed, replay=rec)
    finally:
        torch.set_default_dtype(torch.float32)
    return rec, rec64


def store(out, tag, cls, kw, rec):
    out[f"{tag}_ser"] = np.array(rec["ser"], np.float64)
    out[f"{tag}_errors"] = np.array(rec["errors"], np.int64)
    out[f"{tag}_lr"] = np.array(kw["lr"])
    if cls is VNETTrainer:
        out[f"{tag}_idx"] = np.array(rec["multinomial"], np.uint8).reshape(3, 25, 32)
        out[f"{tag}_loss"] = np.array(rec["loss"], np.float64).reshape(3, 25)
        out[f"{tag}_best"] = np.array(rec["saves"][-1], np.int64)
        digest(rec["final"], f"{tag}_final", out)
        if rec["saves"][-1] != 2:
            digest(rec["saved_weights"][-1], f"{tag}_best", out)
    else:
        out[f"{tag}_randint"] = np.array(rec["randint"], np.int64).reshape(3, 4)
        loss = np.full((3, 4), np.nan)
        for mb in range(3):
            v = [x for m, x in rec["meta_loss"] if m == mb]
            loss[mb, :len(v)] = v
        out[f"{tag}_loss"] = loss
        out[f"{tag}_meta_lr"] = np.array(BASE["meta_lr"])
        assert rec["saves"] == [0, 1, 2]
        assert all(np.array_equal(a, b) for a, b in zip(rec["saved_weights"][2], rec["final"]))
        digest(rec["final"], f"{tag}_final", out)


def main():
    torch.set_num_threads(8)
    for seed in SEEDS:
        recs, ok = {}, True
        for tag, cls, kw in FLOWS:
            rec, rec64 = both_dtypes(cls, kw, seed)
            same = rec["errors"] == rec64["errors"] and rec["saves"] == rec64["saves"]
            moved = max(float(np.abs(a - b).max()) for a, b in zip(rec["final"], rec["w0"]))
            print(f"g22 seed {seed} {tag}: errors {rec['errors']} (float64 {rec64['errors']}), saves {rec['saves']} (float64 "
                  f"{rec64['saves']}), ser {np.round(rec['ser'], 4).tolist()}, weights moved by {moved:.3f}: {'same' if same else 'DIFFERENT'}")
            recs[tag] = rec
            ok = ok and same
            if not same:
                break
        if not ok:
            continue
        first = recs[FLOWS[0][0]]
        for tag, _, _ in FLOWS:  # every flow saw the same words and started from the same weights
            r = recs[tag]
            assert all(np.array_equal(a, b) for a, b in zip(r["w0"], first["w0"]))
            for ph in ("train", "val"):
                assert len(r["words"][ph]) == 3
                assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(r["words"][ph], first["words"][ph]))
        out = {f"w0_{k}": w.astype(np.float32) for k, w in enumerate(first["w0"])}
        for ph in ("train", "val"):
            out[f"{ph}_tx"] = np.stack([w[0] for w in first["words"][ph]])
            out[f"{ph}_rx"] = np.stack([w[1] for w in first["words"][ph]])
        out["meta"] = np.array([seed, WORD_SEED, 2, 25, 10, 4], np.int64)
        for tag, cls, kw in FLOWS:
            store(out, tag, cls, kw, recs[tag])
        path = os.path.join(HERE, "g22_joint_training.npz")
        np.savez_compressed(path, **out)
        print(f"g22: took noise seed {seed}; wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")
        return
    raise SystemExit("no seed of SEEDS gives the same error counts and best minibatch in float32 and float64 for every flow")


if __name__ == "__main__":
    main()
