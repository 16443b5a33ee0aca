"""mvn_vnet_montecarlo_f32 / mvn.vnet_monte_carlo (csrc/vnet_montecarlo.inc): the 16-state ViterbiNet Monte-Carlo point with the
words generated inside the detector, against the two launches it replaces -- mvn.generate_words (the same pure function of
(seed, word, position)) and VNETDetector.val_count -- counter for counter, exactly.

Shapes: T around the super-tile (32 symbols) and around the kernel's refill of 256 generated symbols, B below / at / above a
workgroup's eight waves and a few hundred, one channel row, three (which do not divide B) and one per word.  Weights: the
reference-trained 16-state ViterbiNet of golden G7 (time_decay, gamma 0.2), run at 6 dB so that every shape of 1000 bits or more
has bit errors to count.  The rounds and the stop rule are checked against every round computed alone."""
import numpy as np
import pytest
import torch

import meta_viterbinet_amd as mvn

pytestmark = pytest.mark.gpu

S, L = 16, 4
REFILL = 256  # kMcRefill of csrc/vnet_montecarlo.inc: symbols a wave generates at a time
SNR, GAMMA, SEED = 6.0, 0.2, 20260711
TS = (1, 31, 32, 33, REFILL - 1, REFILL, REFILL + 1, 1000)
BS = (1, 7, 8, 9, 300)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def detector(dev, golden):
    """T -> the G7 detector with 'val' length T (one per length, built once)."""
    g7, made = golden("g7_by_word"), {}

    def get(T, poison=False):
        if (T, poison) not in made:
            det = mvn.VNETDetector(S, {"train": T, "val": T}).to(dev)
            with torch.no_grad():
                for p, k in zip(det.net.parameters(), range(6)):
                    p.copy_(torch.from_numpy(g7[f"w{k}"]))
                if poison:  # a non-finite weight of the last layer: the kernels must take torch.min's NaN-propagating forms
                    det.net[4].weight[3, 7] = float("inf")
            made[(T, poison)] = det
        return made[(T, poison)]

    return get


def channel(Bh):
    """Bh rows of taps: time_decay at gamma 0.2, rows 1.. faded like the reference's fading channel at word index i."""
    return np.concatenate([mvn.estimate_channel(L, GAMMA, "time_decay", fading=i > 0, index=7 * i) for i in range(Bh)], axis=0)


@pytest.fixture(scope="module")
def two_launches(dev, detector):
    """(B, T, Bh, seed, poison) -> (tx, y, counters of val_count over all rows): computed once, shared, never written to."""
    made = {}

    def get(B, T, Bh, seed=SEED, poison=False):
        key = (B, T, Bh, seed, poison)
        if key not in made:
            tx, y = mvn.generate_words(B, T, channel(Bh), SNR, L, dev, seed)
            made[key] = (tx, y, detector(T, poison).val_count(y, tx).tolist())
        return made[key]

    return get


def check_counters(got, want, B, T, tag):
    print(f"{tag}: B {B} T {T} one launch {got} two launches {want}")
    assert got == want, f"{tag}: counters differ from generate_words + val_count"
    assert got[1] == B * T and got[3] == B
    assert got[2] <= B and got[0] >= got[2]


@pytest.mark.parametrize("Bh_kind", ("one", "three", "per_word"))
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
def test_counters_equal_the_two_launches(dev, detector, two_launches, T, B, Bh_kind):
    Bh = {"one": 1, "three": 3, "per_word": B}[Bh_kind]
    want = two_launches(B, T, Bh)[2]
    got = mvn.vnet_monte_carlo(detector(T), B, channel(Bh), SNR, dev, SEED).tolist()
    check_counters(got, want, B, T, f"Bh {Bh}")
    if B * T >= 1000:  # a detector at work: errors, and far fewer than a coin's
        assert 0 < got[0] < B * T / 4, f"{got[0]} bit errors in {B * T} bits"


@pytest.mark.parametrize("B,T", ((9, 100), (3, 300)))  # (more than a workgroup's waves; across a refill)
def test_a_non_finite_weight_follows_torch_min_on_both_routes(dev, detector, two_launches, B, T):
    want = two_launches(B, T, 3, poison=True)[2]
    got = mvn.vnet_monte_carlo(detector(T, True), B, channel(3), SNR, dev, SEED).tolist()
    check_counters(got, want, B, T, "inf in W3")
    assert got != two_launches(B, T, 3)[2], "the poisoned weight changed nothing: the case tests nothing"


def test_counters_accumulate_and_follow_the_seed(dev, detector, two_launches):
    B, T = 300, 257
    det, h = detector(T), channel(3)
    first = mvn.vnet_monte_carlo(det, B, h, SNR, dev, SEED)
    once = first.tolist()
    assert once == two_launches(B, T, 3)[2]
    again = mvn.vnet_monte_carlo(det, B, h, SNR, dev, SEED, counters=first)
    assert again is first and again.tolist() == [2 * c for c in once]
    other = mvn.vnet_monte_carlo(det, B, h, SNR, dev, SEED + 1).tolist()
    assert other == two_launches(B, T, 3, seed=SEED + 1)[2]
    assert other[0] != once[0] and other[1] == once[1]


def test_first_word_addresses_the_global_sequence(dev, detector, two_launches):
    """Three uneven shards of 300 words (what three ranks would run) sum to the whole point, and each equals its rows of the two
    launches; the three channel rows make a shard that started its rows at 0 visible."""
    B, T = 300, 257
    det, h = detector(T), channel(3)
    tx, y, whole = two_launches(B, T, 3)
    total = torch.zeros(4, dtype=torch.int64, device=dev)
    for lo, hi in ((0, 97), (97, 201), (201, 300)):
        got = mvn.vnet_monte_carlo(det, hi - lo, h, SNR, dev, SEED, first_word=lo).tolist()
        check_counters(got, det.val_count(y[lo:hi], tx[lo:hi]).tolist(), hi - lo, T, f"words {lo}:{hi}")
        mvn.vnet_monte_carlo(det, hi - lo, h, SNR, dev, SEED, first_word=lo, counters=total)
    assert total.tolist() == whole
    assert mvn.vnet_monte_carlo(det, 99, h, SNR, dev, SEED, first_word=201).tolist() != mvn.vnet_monte_carlo(det, 99, h, SNR, dev, SEED).tolist()


ROUNDS, PER_ROUND, T_ROUNDS = 12, 64, 100


@pytest.fixture(scope="module")
def single_rounds(dev, detector):
    """The 12 rounds of 64 words, each computed alone (rounds=1, first_word = 64 r): [12][4] integers."""
    det, h = detector(T_ROUNDS), channel(3)
    return [mvn.vnet_monte_carlo(det, PER_ROUND, h, SNR, dev, SEED, first_word=r * PER_ROUND).tolist() for r in range(ROUNDS)]


def staged(dev, detector, F, **kw):
    counters, rounds_run = mvn.vnet_monte_carlo(detector(T_ROUNDS), PER_ROUND, channel(3), SNR, dev, SEED, rounds=ROUNDS, stop_frame_errors=F, **kw)
    assert rounds_run.device.type == "cuda" and rounds_run.dtype == torch.int32
    return counters.tolist(), int(rounds_run.item())


def sum_rounds(rounds):
    return [sum(r[i] for r in rounds) for i in range(4)]


def test_rounds_without_a_stop_rule_run_all(dev, detector, single_rounds, two_launches):
    assert sum_rounds(single_rounds) == two_launches(ROUNDS * PER_ROUND, T_ROUNDS, 3)[2]  # the rounds tile the sequence
    got, ran = staged(dev, detector, 0)
    assert ran == ROUNDS and got == sum_rounds(single_rounds)


def test_stop_rule_runs_whole_rounds_up_to_the_target(dev, detector, single_rounds):
    fe = np.cumsum([r[2] for r in single_rounds])
    print("frame errors per round", [r[2] for r in single_rounds])
    assert all(r[2] > 0 for r in single_rounds), "an SNR at which single rounds have frame errors"
    F = int(fe[4]) + 1  # reached in the sixth round: strictly inside the sequence
    k = int(np.argmax(fe >= F)) + 1  # the first round count whose cumulative frame errors reach F (from the single rounds alone)
    assert 1 < k < ROUNDS and fe[k - 1] >= F > fe[k - 2] and fe[-1] > F
    want = sum_rounds(single_rounds[:k])
    got, ran = staged(dev, detector, F)
    print(f"F {F}: ran {ran} rounds, counters {got}; first {k} single rounds {want}")
    assert ran == k and got == want
    assert staged(dev, detector, F) == (got, ran), "a repetition gave other integers"
    # a target met exactly at a round's end stops there, one more frame error asks for another round
    assert staged(dev, detector, int(fe[k - 1])) == (want, k)
    assert staged(dev, detector, int(fe[k - 1]) + 1) == (sum_rounds(single_rounds[:k + 1]), k + 1)
    # a target beyond the sequence: every round runs
    assert staged(dev, detector, int(fe[-1]) + 1) == (sum_rounds(single_rounds), ROUNDS)


def test_stop_rule_sees_the_counters_it_is_given(dev, detector, single_rounds):
    """The gate compares what the counters hold, so a point is resumed by passing them back: nothing runs once the target is met."""
    fe = np.cumsum([r[2] for r in single_rounds])
    F = int(fe[2])
    first, ran = staged(dev, detector, F)
    assert ran == 3 and first == sum_rounds(single_rounds[:3])
    c = torch.tensor(first, dtype=torch.int64, device=dev)
    assert staged(dev, detector, F, counters=c, first_word=3 * PER_ROUND) == (first, 0)
    more, ran = staged(dev, detector, int(fe[4]), counters=c, first_word=3 * PER_ROUND)
    assert ran == 2 and more == sum_rounds(single_rounds[:5])
