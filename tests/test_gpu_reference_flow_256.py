"""GPU: the reference's own by-word flow with self-supervised training at channel memory 8 (256 states), replayed draw for draw
(golden G23, tests/golden/make_golden_256_states.py: train_vnet(8, 10), then 50 blocks of the unmodified VNETTrainer's
eval_by_word with 8 minibatch iterations per qualifying block, RS(17, 15), recorded with ser_thresh = 0.12 -- the briefly trained
256-state detector sits near ser 0.10, under the default 0.02 three blocks would train; the fixture carries the threshold).
mvn.eval_by_word runs the same words on online_train_kernel<256, false> and on the torch-autograd route of the same host code
(the control: that route is what every earlier version ran at 256 states).  What must come out, as in
test_reference_by_word_flow_other_state_counts: the reference's ser_by_word on all 50 blocks (the ser decides which blocks train,
so one differing block misaligns the recorded draws), every recorded draw used up, weights that moved, and final weights within
5e-5 of the reference's."""
import ctypes

import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn
from test_gpu_reference_flow import RecordedDraws

pytestmark = pytest.mark.gpu
TAG = "L8_selfsup"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.mark.parametrize("route", ["hip_kernels", "torch_autograd"])
def test_reference_by_word_flow_at_256_states(golden, dev, route):
    g = golden("g23_by_word_256_states")
    hip = route == "hip_kernels"
    ss_it, _, _, _, snr, subframes, nsym = [int(v) for v in g[f"{TAG}_meta"]]
    ser_thresh = float(g[f"{TAG}_ser_thresh"])
    ref = g[f"{TAG}_ser_by_word"]
    assert ser_thresh == 0.12 and not np.any(ref == ser_thresh) and 10 < int((ref <= ser_thresh).sum()) < 50
    tx = torch.tensor(g[f"{TAG}_tx"], device=dev).float()
    rx = torch.tensor(g[f"{TAG}_rx"], device=dev)
    T = rx.shape[1]
    w0 = [g[f"{TAG}_w0_{i}"] for i in range(6)]
    S = w0[5].shape[0]
    assert S == 256 and T == 136
    det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
    with torch.no_grad():
        for p, a in zip(det.parameters(), w0):
            p.copy_(torch.as_tensor(a))
    tr = mvn.OnlineTrainer(det, 8, use_kernel=hip)
    if hip:
        name = ctypes.create_string_buffer(96)
        assert mvn._lib.load().mvn_vnet_train_kernel_name(0, 0, T, tr.train_minibatch_size, S, 0, name, 96) == 0
        assert name.value.decode() == "online_train_kernel<256, false> 1x1"
    draws = RecordedDraws(g[f"{TAG}_multinomial"], g[f"{TAG}_randint_high"], g[f"{TAG}_randint"], dev)
    ser = mvn.eval_by_word(det, tx, rx, float(snr), 0.2, nsym, subframes, online_trainer=tr, draws=draws, hip_meta=hip, graphed_meta=False,
                           self_supervised=True, self_supervised_iterations=ss_it, ser_thresh=ser_thresh)
    w = [p.detach().cpu().numpy() for p in det.parameters()]
    assert ser.shape == ref.shape == (50,)
    assert np.array_equal(ser, ref), (np.flatnonzero(ser != ref), ser[ser != ref], ref[ser != ref])
    assert draws.used_up(), (draws.m_at, len(draws.multinomial), draws.r_at, len(draws.randint))
    assert tr.step == len(g[f"{TAG}_multinomial"]) == ss_it * int((ref <= ser_thresh).sum())
    moved = max(float(np.abs(g[f"{TAG}_w1_{i}"] - w0[i]).max()) for i in range(6))
    worst = max(float(np.abs(w[i] - g[f"{TAG}_w1_{i}"]).max()) for i in range(6))
    print(f"g23 {TAG} (256 states) {route}: ser identical on 50 blocks; weights moved {moved:.4f}, end {worst:.2e} from the reference's")
    assert moved > 0.005 and worst <= 5e-5
