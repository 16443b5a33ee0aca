#!/usr/bin/env python3
"""G18 generator (the LSTM detector): imports the UNMODIFIED reference on CPU, like make_golden.py, and writes
tests/golden/g18_lstm.npz:

    MVN_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_lstm.py

  w{i}, w_exp the ten parameters of a reference-trained LSTMDetector (LSTMTrainer.train, small hyperparameters, fixed seed) in
              parameters() order, rounded to int8 multiples of a power-of-two step per tensor: w{i} * 2**w_exp[i] is exact in f32
              (bf16 patterns would be 1.6 MB, over the size limit of a committed file); every output below is the reference's
              on exactly these values
  keys/shapes the state_dict key list and shapes
  tx, rx      the words single_eval_at_point drew from the reference's val channel (100 words, 10 dB, RS nsym 2: T = 136)
  logits      LSTMDetector(rx, 'train');  dec: LSTMDetector(rx, 'val');  dec_meta: MetaLSTMDetector(rx, 'val', var = the weights)
  ser         Trainer.single_eval_at_point's ser on those words; data_indices: the rows it counts
"""
import math
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
TMP = tempfile.mkdtemp(prefix="mvn_golden_lstm_")

from python_code.detectors.LSTM.lstm_detector import LSTMDetector  # noqa: E402
from python_code.detectors.META_LSTM.meta_lstm_detector import MetaLSTMDetector  # noqa: E402
from python_code.trainers.LSTM.lstm_trainer import LSTMTrainer  # noqa: E402


def quantize(t: torch.Tensor):
    """int8 multiples of the power-of-two step that fits the tensor's largest magnitude in 127 steps: (q, exponent)."""
    m = float(t.detach().abs().max())
    e = math.ceil(math.log2(m / 127)) if m > 0 else 0
    return torch.clamp(torch.round(t.detach() / 2.0 ** e), -127, 127).to(torch.int8).numpy(), e


def dequantize(q: np.ndarray, e: int) -> np.ndarray:
    return q.astype(np.float32) * np.float32(2.0 ** e)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(1818)
    kw = dict(use_ecc=True, n_symbols=2, memory_length=4, val_block_length=120, val_frames=4, subframes_in_frame=25,
              train_block_length=120, train_frames=1, train_minibatch_num=3, train_minibatch_size=32,
              channel_coefficients="time_decay", fading_in_channel=False, fading_in_decoder=False, noisy_est_var=0,
              train_SNR_start=10, train_SNR_end=10, val_SNR_start=10, val_SNR_end=10, gamma=0.2, lr=1e-3,
              optimizer_type="Adam", loss_type="CrossEntropy", self_supervised=False, online_meta=False, eval_mode="aggregated",
              noise_seed=3450002, word_seed=7860002, weights_dir=TMP)
    tr = LSTMTrainer(**kw)
    tr.train()
    ck = torch.load(os.path.join(TMP, "snr_10_gamma_0.2.pt"))
    det = LSTMDetector()
    det.load_state_dict(ck["model_state_dict"])
    qs = [quantize(p) for p in det.parameters()]
    with torch.no_grad():
        for p, (q, e) in zip(det.parameters(), qs):
            p.copy_(torch.from_numpy(dequantize(q, e)))
    # the words of one evaluation: a fresh trainer (same seeds) whose val dataset draw is recorded
    ev = LSTMTrainer(**kw)
    ev.detector = det
    seen = {}
    orig = ev.channel_dataset["val"].__getitem__

    def spy(snr_list, gamma, _f=orig):
        seen["tx"], seen["rx"] = _f(snr_list=snr_list, gamma=gamma)
        return seen["tx"], seen["rx"]

    ev.channel_dataset["val"].__getitem__ = spy
    with torch.no_grad():
        ser = ev.single_eval_at_point(10, 0.2)
        rx = seen["rx"]
        logits = det(rx, "train")
        dec = det(rx, "val")
        dec_meta = MetaLSTMDetector()(rx, "val", list(det.parameters()))
    sd = det.state_dict()
    out = {f"w{i}": q for i, (q, _) in enumerate(qs)}
    out["w_exp"] = np.array([e for _, e in qs], np.int64)
    out.update(keys=np.array(list(sd.keys())), shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64),
               tx=seen["tx"].numpy().astype(np.uint8), rx=rx.numpy(), logits=logits.numpy(), dec=dec.numpy().astype(np.uint8),
               dec_meta=dec_meta.numpy().astype(np.uint8), ser=np.array(ser, np.float64), data_indices=ev.data_indices.numpy(),
               meta=np.array([4, 2, 10], np.int64))  # memory length, n_symbols, snr
    path = os.path.join(HERE, "g18_lstm.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB); ser {ser}; meta == lstm: {np.array_equal(dec, dec_meta)}")


if __name__ == "__main__":
    main()
