"""CPU checks of tests/exact_nets.py: the C oracle against a second, independent reference (a float64 step-function MLP and a
NumPy textbook Viterbi) bit for bit on the tie-heavy staircase networks; the preconditions that make those inputs able to catch
a wrong tie rule; and that the sigmoid-range and subnormal inputs reach what they are meant to reach.  No GPU."""
import numpy as np
import pytest

import exact_nets as E

STATES = [2, 4, 8, 16, 32, 64, 128, 256]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("S", STATES)
def test_oracle_equals_ideal_mlp_and_textbook_viterbi(oracle, S, fast, strict):
    """oracle.vnet_decode == ideal_logits + textbook_acs(-logits): logits, decisions, final metrics; oracle.acs_sweep_surv and
    oracle.traceback == the textbook survivors and path.  Every comparison is exact."""
    for B, T in E.TIE_SHAPES[S][:2]:
        c = E.tie_case(S, fast, strict, B, T)
        bound = np.abs(c["y"]).max() * np.abs(c["w"][0]).max() + np.abs(c["w"][1]).max()
        assert (bound <= 86.0) == fast and bound == (64.0 if fast else 576.0)  # which sigmoid form the kernels' tiles take
        assert (np.abs(c["w"][3]).max() >= 1e14) == strict
        dec, lg, fm = oracle.vnet_decode(c["y"], c["w"], want_logits=True, want_final=True)
        assert np.array_equal(lg, c["logits"])
        assert np.array_equal(dec, c["dec"]) and np.array_equal(fm, c["fm"])
        assert np.all(dec[:, 0] == 0)  # quirk Q1
        dec2, fm2, surv = oracle.acs_sweep_surv(-c["logits"])
        assert np.array_equal(dec2, c["dec"]) and np.array_equal(fm2, c["fm"])
        assert surv.shape == c["surv"].shape and np.array_equal(surv, c["surv"])
        bits, states = oracle.traceback(surv, fm2)
        assert np.array_equal(bits, c["path"]) and np.array_equal(states & 1, c["path"].astype(np.int32))


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("S", STATES)
def test_tie_preconditions(S, fast, strict):
    """Every (B, T) the GPU tests use, at its hard-coded seed: at least 1 % of the decisions after symbol 0 and 1 % of the survivor
    bits depend on the tie rule, both decision values occur (S = 2 decides 0 throughout: its two states always tie), and the path
    metrics are exact in f32."""
    for B, T in E.TIE_SHAPES[S]:
        p = E.tie_preconditions(S, fast, strict, B, T)
        assert p["dec_ties"] >= 0.01, (B, T, p)
        assert p["surv_ties"] >= 0.01, (B, T, p)
        assert S == 2 or 0.1 <= p["ones"] <= 0.9, (B, T, p)
        assert p["exact"] < 2 ** 24, (B, T, p)


def test_staircase_layer1_is_an_exact_step(oracle):
    """What ideal_logits assumes of layer 1, from the oracle's own sigmoid: at the arguments the staircase networks produce
    (|z| >= 64, up to 576) it is 1.0f exactly or at most e^-64."""
    z = np.array([64.0, 128.0, 192.0, 576.0], np.float32)
    assert np.all(oracle.sigmoid(z) == 1.0)
    lo = oracle.sigmoid(-z)
    assert np.all(lo >= 0.0) and np.all(lo <= np.float32(1.7e-28)) and lo[3] == 0.0


def test_textbook_acs_tie_rules():
    """Two stages by hand at 4 states, all costs equal: every comparison ties; first-index and last-index rules as stated."""
    cost = np.zeros((1, 2, 4), np.float32)
    dec, fm, surv, path = E.textbook_acs(cost)
    assert dec.tolist() == [[0, 0]] and surv[0, :, 0].tolist() == [0, 0] and path.tolist() == [[0, 0]] and not fm.any()
    dec, fm, surv, path = E.textbook_acs(cost, last=True)
    assert dec.tolist() == [[1, 1]] and surv[0, :, 0].tolist() == [15, 15] and path.tolist() == [[1, 1]]
    cost[0, 0] = [3, 1, 2, 2]  # state 0 <- min(3, 1): index 1; state 1 <- min(2, 2): tie; states 2, 3 the same
    dec, fm, surv, _ = E.textbook_acs(cost)
    assert fm.tolist() == [[1, 1, 1, 1]] and surv[0, 0, 0] == 0b0101 and surv[0, 1, 0] == 0  # (stage 2: min(1, 2) twice)
    assert E.textbook_acs(cost, last=True)[2][0, 0, 0] == 0b1111


@pytest.mark.parametrize("S", [4, 16, 256])
def test_ladder_inputs_reach_both_forms_and_the_subnormal_range(oracle, S):
    """Row 0's tiles alternate between the two sigmoid forms with 86.0 exactly on the switch; one hidden-1 unit's argument is
    -rung itself, which at 87.5 and 88.5 makes the oracle's sigmoid subnormal; the oracle's logits stay finite up to 3e38."""
    w = E.ladder_weights(S, np.random.RandomState(S))
    y = E.ladder_samples(9, 200, np.random.RandomState(S + 1))
    wmax, bmax = np.abs(w[0]).max(), np.abs(w[1]).max()
    bound = (np.abs(y[0, :192]).reshape(12, 16).max(axis=1) * wmax + bmax).astype(np.float32)
    assert bound[1] == np.float32(86.0) and np.float32(85.8) < bound[3] < np.float32(86.0)
    assert np.all(bound[[0, 2, 4, 6, 8, 10]] > 86.0) and np.all(bound[[5, 7, 9, 11]] < 86.0)
    k = int(np.argmax(np.abs(w[0])))
    z = (y * w[0][k, 0] + w[1][k]).astype(np.float32)
    tiny = np.float32(2.0 ** -126)
    for rung in (87.5, 88.5):
        s = oracle.sigmoid(np.array([-rung], np.float32))[0]
        assert 0.0 < s < tiny and np.any(z[0] == np.float32(-rung)) and np.any(z[1:] == np.float32(-rung))
    assert oracle.sigmoid(np.array([-87.0], np.float32))[0] >= tiny and oracle.sigmoid(np.array([-104.5], np.float32))[0] == 0.0
    for r in E.LADDER_RUNGS:  # every rung occurs, with either sign of y
        v = np.float32((r - E.LADDER_BMAX) / E.LADDER_WMAX)
        assert np.any(y == v) and np.any(y == -v), r
    assert np.any((y == 0) & np.signbit(y)) and np.any(y == np.float32(1e-40))
    assert np.isfinite(oracle.vnet_logits(y, w)).all()


@pytest.mark.parametrize("k,j", E.SUBNORMAL_KJ)
def test_subnormal_activation_decides_logits_and_decisions(oracle, k, j):
    """oracle.sigmoid(-88) is subnormal; the oracle's logits on the y = 1.0 samples are 2^80 times that value where a flushed
    activation gives 0, and the decisions of the all-1.0 block are 1 where a flushed activation gives 0: the case can fail."""
    S, B, T = 16, 5, 75
    h = oracle.sigmoid(np.array([-88.0], np.float32))[0]
    assert h == np.float32(6.054601e-39) and 0.0 < h < np.float32(2.0 ** -126)
    w = E.subnormal_net(S, k, j, np.random.RandomState(100 * k + j))
    assert max(np.abs(a).max() for a in w) < 1e14  # below kStrictMinBound
    y = E.subnormal_samples(B, T, np.random.RandomState(k + j))
    dec, lg = oracle.vnet_decode(y, w, want_logits=True)
    dec0, lg0 = oracle.vnet_decode(y, E.flushed(w, k, j), want_logits=True)
    half = (np.arange(S) & 2) != 0
    sub = y == 1.0
    assert 0.2 < sub[1:].mean() < 0.8
    assert np.all(lg[sub][:, half] == h * np.float32(2.0 ** 80)) and np.all(lg0[sub][:, half] == 0.0)
    assert np.all(lg[~sub][:, half] > 1e4)  # the normal activation of y = 0.5
    assert np.array_equal(lg[:, :, ~half], lg0[:, :, ~half]) and np.all(lg[:, :, 0] == 0.0) and np.all(lg[:, :, ~half][:, :, 1:] < -1.0)
    assert np.all(dec[0, 1:] == 1.0) and np.all(dec0[0] == 0.0)
