#!/usr/bin/env python3
"""G20 generator (online meta-learning of the LSTM detector, the Meta-LSTM curve): imports the UNMODIFIED reference on CPU, like
make_golden_lstm_train.py, starts from G18's committed weights and writes tests/golden/g20_lstm_meta.npz:

    MVN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_lstm_meta.py

Final weights are stored as G19's digest (the four small tensors whole; of the six big ones 4096 entries at positions drawn by
numpy.random.RandomState(1900 + k).choice(size, 4096, replace=False) and the L2 norm).

  a_*  4 calls of Trainer.meta_train_loop (trainer.py:425-453) as MetaLSTMTrainer with MAML=True, meta_lr 0.1: call w takes G18 word
       w as the support word and word w + 1 as the query word.  a_tx (the RS codewords of words 0 .. 4), a_rx, a_loss (the query
       losses), the digest a_p{k} / a_n{k}
  b_*  the same with MAML=False: b_loss, digest
  c_*  one MetaLSTMTrainer.evaluate() by word with online_meta=True, MAML=False, self_supervised=True (one frame of 25 blocks,
       10 dB), cut down so that it runs in minutes on a CPU and in seconds in the tests:
       meta_train_iterations 2, meta_j_num 3, self_supervised_iterations 4, meta_subframes 5.  c_tx, c_rx the words, c_randint /
       c_randint_high every torch.randint draw of trainer.py:337 in call order, c_ser_by_word, c_trained (which blocks trained),
       c_meta_blocks (which blocks ran a meta update), c_min_margin / c_margin_band as in G19 (the float64 rerun replays the draws),
       c_meta = [self_supervised_iterations, subframes_in_frame, n_symbols, snr, noise_seed, meta_train_iterations, meta_j_num,
       meta_subframes], c_ser_thresh, c_meta_lr, digest c_p{k} / c_n{k} of the detector's weights after the run.  The seed is the
       first of SEEDS with >= 3 meta updates, >= 5 trained blocks, the same control flow in float64 and <= 10 % of the data blocks
       exempt by margin.
"""
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
TMP = tempfile.mkdtemp(prefix="mvn_golden_lstm_meta_")

from python_code.ecc.rs_main import encode  # noqa: E402
from python_code.trainers.META_LSTM.meta_lstm_trainer import MetaLSTMTrainer  # noqa: E402

SER_THRESH = 0.1  # as in G19: G18's weights decode these words at a mean ser of 0.1
META_LR = 0.1
SS_ITERS, META_ITERS, META_J, META_SUBFRAMES = 4, 2, 3, 5
SEEDS = (3450002, 3450003, 3450004, 3450005, 3450006, 3450007)
BASE = dict(use_ecc=True, n_symbols=2, memory_length=4, val_block_length=120, val_frames=1, subframes_in_frame=25,
            train_block_length=120, train_frames=1, train_minibatch_num=1, train_minibatch_size=32,
            channel_coefficients="time_decay", fading_in_channel=False, fading_in_decoder=False, noisy_est_var=0,
            train_SNR_start=10, train_SNR_end=10, val_SNR_start=10, val_SNR_end=10, gamma=0.2, lr=1e-3,
            optimizer_type="Adam", loss_type="CrossEntropy", buffer_empty=True, ser_thresh=SER_THRESH, word_seed=7860002,
            meta_lr=META_LR, window_size=1, weights_init="last_frame", meta_train_iterations=META_ITERS, meta_j_num=META_J,
            meta_subframes=META_SUBFRAMES)


def g18_weights():
    g = np.load(os.path.join(HERE, "g18_lstm.npz"))
    return g, [g[f"w{i}"].astype(np.float32) * np.float32(2.0 ** int(g["w_exp"][i])) for i in range(10)]


def load_into(det, ws):
    with torch.no_grad():
        for p, w in zip(det.parameters(), ws):
            p.copy_(torch.from_numpy(w).to(p.dtype))


def digest(det, prefix, out):
    for k, p in enumerate(det.parameters()):
        w = p.detach().double().numpy().reshape(-1)
        if w.size <= 4096:
            out[f"{prefix}p{k}"] = w
        else:
            pos = np.random.RandomState(1900 + k).choice(w.size, 4096, replace=False)
            out[f"{prefix}p{k}"] = w[pos]
            out[f"{prefix}n{k}"] = np.array(np.linalg.norm(w))


def part_a_b(out, g, ws):
    tx = torch.cat([torch.Tensor(encode(g["tx"][w].astype(int), 2).reshape(1, -1)) for w in range(5)], dim=0)
    rx = torch.from_numpy(g["rx"][:5].copy())
    out.update(a_tx=tx.numpy().astype(np.uint8), a_rx=rx.numpy())
    for part, maml in (("a", True), ("b", False)):
        torch.manual_seed(2001)
        tr = MetaLSTMTrainer(**BASE, MAML=maml, online_meta=True, self_supervised=True, self_supervised_iterations=SS_ITERS,
                             eval_mode="by_word", noise_seed=SEEDS[0], weights_dir=TMP)
        load_into(tr.detector, ws)
        tr.deep_learning_setup()
        losses = [float(tr.meta_train_loop(rx, tx, torch.tensor([w]), torch.tensor([w + 1])).detach()) for w in range(4)]
        out[f"{part}_loss"] = np.array(losses, np.float64)
        digest(tr.detector, f"{part}_", out)
        print(f"g20 {part}: MAML={maml}: query losses", losses)


def by_word_run(ws, noise_seed, replay=None):
    """One evaluate() by word: (tx, rx, ser_by_word, randint draws [(high, values)], trained blocks, meta blocks, per-block logits,
    the trainer)."""
    wdir = os.path.join(TMP, f"w_c_{noise_seed}_{torch.get_default_dtype()}")
    os.makedirs(wdir, exist_ok=True)
    kw = dict(BASE, MAML=False, online_meta=True, self_supervised=True, self_supervised_iterations=SS_ITERS, eval_mode="by_word",
              noise_seed=noise_seed, weights_dir=wdir)
    torch.manual_seed(2002)
    tr = MetaLSTMTrainer(**kw)
    sd = tr.detector.state_dict()
    for k, w in zip(list(sd.keys()), ws):
        sd[k] = torch.from_numpy(w)
    torch.save({"model_state_dict": sd, "optimizer_state_dict": {}, "loss": 0.0}, os.path.join(wdir, "snr_10_gamma_0.2.pt"))
    tx_msg, rx = tr.channel_dataset["val"].__getitem__(snr_list=[10], gamma=0.2)  # same seeds -> the words evaluate() will draw
    tr2 = MetaLSTMTrainer(**kw)
    logits, trained, meta_blocks, draws = [], [], [], []
    det_cls = type(tr2.detector)
    real_forward, real_online, real_init, real_randint = det_cls.forward, tr2.online_training, tr2.meta_weights_init, torch.randint

    def fspy(self_, y, phase, *a, **k):
        if phase == "val" and self_ is tr2.detector:
            with torch.no_grad():
                logits.append(real_forward(self_, y, "train")[0].double().numpy().copy())
        return real_forward(self_, y, phase, *a, **k)

    def ospy(tx, rx):
        trained.append(len(logits) - 1)
        return real_online(tx, rx)

    def ispy():
        meta_blocks.append(len(logits) - 1)
        return real_init()

    def rspy(*a, **k):
        r = real_randint(*a, **k)
        if "high" not in k:  # (not trainer.py:337's call)
            return r
        if replay is not None:
            high, values = replay[len(draws)]
            assert high == int(k["high"])
            r = torch.from_numpy(values.astype(np.int64))
        draws.append((int(k["high"]), r.numpy().copy()))
        return r

    det_cls.forward, tr2.online_training, tr2.meta_weights_init, torch.randint = fspy, ospy, ispy, rspy
    try:
        ser = tr2.evaluate()
    finally:
        det_cls.forward, torch.randint = real_forward, real_randint
    return tx_msg.numpy(), rx.numpy(), np.asarray(ser, np.float64), draws, trained, meta_blocks, np.stack(logits), tr2


def part_c(out, ws):
    import contextlib
    import io

    for seed in SEEDS:
        with contextlib.redirect_stdout(io.StringIO()):
            tx, rx, ser, draws, trained, metas, lg, tr = by_word_run(ws, seed)
            torch.set_default_dtype(torch.float64)
            try:
                same_flow = True
                try:
                    _, _, ser64, draws64, trained64, metas64, lg64, _ = by_word_run(ws, seed, replay=draws)
                except (AssertionError, IndexError):  # another buffer length: the float64 run has parted from this one
                    same_flow = False
            finally:
                torch.set_default_dtype(torch.float32)
        same_flow = same_flow and trained == trained64 and metas == metas64 and len(draws) == len(draws64)
        band = 100.0 * float(np.abs(lg - lg64).max()) if same_flow else float("inf")
        min_margin = np.abs(lg[..., 1] - lg[..., 0]).min(axis=1)
        data = np.arange(len(ser)) % 25 != 0
        exempt = int((min_margin[data] < band).sum())
        print(f"g20 c: noise seed {seed}: {len(trained)} blocks trained, {len(metas)} meta updates ({len(draws)} randint draws), same "
              f"flow in float64: {same_flow}, margin_band {band:.3g}, exempt data blocks {exempt} of {int(data.sum())}, mean ser "
              f"{ser.mean():.4g}")
        if same_flow and len(metas) >= 3 and len(trained) >= 5 and exempt <= 0.1 * data.sum():
            out.update(c_tx=tx.astype(np.uint8), c_rx=rx.astype(np.float32), c_randint_high=np.array([h for h, _ in draws], np.int64),
                       c_randint=np.array([v for _, v in draws], np.int64).reshape(len(draws), META_J), c_ser_by_word=ser,
                       c_trained=np.array(trained, np.int64), c_meta_blocks=np.array(metas, np.int64), c_min_margin=min_margin,
                       c_margin_band=np.array(band),
                       c_meta=np.array([SS_ITERS, 25, 2, 10, seed, META_ITERS, META_J, META_SUBFRAMES], np.int64),
                       c_ser_thresh=np.array(SER_THRESH), c_meta_lr=np.array(META_LR))
            digest(tr.detector, "c_", out)
            return
    raise SystemExit("no seed of SEEDS gives >= 3 meta updates and >= 5 trained blocks with <= 10 % of the data blocks exempt")


def main():
    torch.set_num_threads(8)
    g, ws = g18_weights()
    out = {}
    part_a_b(out, g, ws)
    part_c(out, ws)
    path = os.path.join(HERE, "g20_lstm_meta.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
