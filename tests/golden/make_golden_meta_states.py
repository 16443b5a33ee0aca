#!/usr/bin/env python3
"""Golden G21: the unmodified reference's eval_by_word as METAVNETTrainer at channel memories 6 and 7 (64 and 128 states), recorded
like G16's meta-learning flows by make_golden.py's _by_word_flow: 6 self-supervised whole-word iterations per block from the saved
weights, every 5 blocks 2 x 4 second-order meta-learning steps (meta_lr 0.1), 50 blocks on a static channel.  The runs start from
the weights G17 recorded (L6_selfsup_w0_* / L7_selfsup_w0_*: the reference's own trainer produced them).  Run where the reference
is available, like make_golden.py:

    PYTHONPATH=<reference> PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_meta_states.py

Writes tests/golden/g21_by_word_meta_64_128_states.npz (maml_train_kernel<64 | 128, false>; tests/test_gpu_maml_states.py)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    from python_code.trainers.META_VNET.metavnet_trainer import METAVNETTrainer

    g17 = np.load(os.path.join(HERE, "g17_by_word_64_128_states.npz"))
    meta = dict(self_supervised=True, self_supervised_iterations=6, online_meta=True, MAML=True, meta_lr=0.1, window_size=1,
                meta_train_iterations=2, meta_j_num=4, meta_subframes=5, weights_init="last_frame")
    out = {}
    for L in (6, 7):
        w = [g17[f"L{L}_selfsup_w0_{i}"] for i in range(6)]
        mg._by_word_flow(out, f"L{L}_meta", METAVNETTrainer, dict(meta, memory_length=L, fading_in_channel=False), None, 2, weights=w)
        tag = f"L{L}_meta"
        ser = out[f"{tag}_ser_by_word"]
        moved = max(float(np.abs(out[f"{tag}_w1_{i}"] - w[i]).max()) for i in range(6))
        moved_s = max(float(np.abs(out[f"{tag}_saved_{i}"] - w[i]).max()) for i in range(6))
        print(f"g21 {tag}: {len(out[f'{tag}_randint'])} randint draws, final weights {moved:.3f} and saved weights {moved_s:.3f} from the "
              f"start, {int((ser > 0).sum())} of {len(ser)} blocks with bit errors")
    mg.save("g21_by_word_meta_64_128_states", **out)


if __name__ == "__main__":
    main()
