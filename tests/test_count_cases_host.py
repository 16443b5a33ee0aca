"""CPU-only: the case builder of count_cases.py against the CPU oracle's count_errors, the geometries it claims, and the proof that
the comparisons of tests/test_gpu_count_errors.py flag a wrong kernel -- shown on the cases themselves, without running one."""
import numpy as np
import pytest
import torch

import count_cases as CC


def numpy_counters(dec, tx, K):
    wrong = dec.astype(np.int64) != tx.astype(np.int64)
    return [int(wrong.sum()), dec.shape[0] * K, int(wrong.any(axis=1).sum()), dec.shape[0]]


@pytest.mark.parametrize("K", CC.KS)
def test_expected_counters_are_the_oracles(oracle, K):
    seen = set()
    for tag, d_off, t_off, ld_d, ld_t in CC.geometries(K):
        c = CC.Case(d_off, t_off, ld_d, ld_t, CC.N_ROWS, K)
        dec, tx = np.ascontiguousarray(c.dec), np.ascontiguousarray(c.tx)
        assert c.expected() == numpy_counters(dec, tx, K) == oracle.count_errors(dec, tx).tolist(), tag
        for i in range(c.n):
            assert c.expected([i]) == oracle.count_errors(dec, tx, [i]).tolist(), (tag, i)
            assert np.flatnonzero(dec[i] != tx[i]).tolist() == c.wrong[i], (tag, i)
            seen.add(c.path(i)[0])
        # the fill: every float outside the rows mismatches, FRONT floats of it in front, between (where rows are apart) and behind
        for buf, view, fill, which in ((c.dec_buf, c.dec, 1.0, "dec"), (c.tx_buf, c.tx, 0.0, "tx")):
            inside = np.zeros(buf.size, bool)
            for i in range(c.n):
                s = c.start[which] + i * c.ld[which]
                inside[s:s + K] = True
                assert np.shares_memory(view[i], buf[s:s + K]) and view[i].ctypes.data == buf[s:].ctypes.data
            assert np.all(buf[~inside] == fill) and not inside[:CC.FRONT].any() and not inside[-CC.FRONT:].any()
            assert c.ld[which] >= K + 32 and set(np.unique(buf[inside])) <= {0.0, 1.0}
        assert np.all(c.dec_buf[:CC.FRONT].astype(np.int64) != c.tx_buf[:CC.FRONT].astype(np.int64))
        # the patterns that exist at this K are there
        assert c.errors[0] == 0 and c.wrong[1] == [0] and c.wrong[2] == [K - 1] and c.errors[6] == K
        assert c.wrong[3] == ([4 * (K // 4)] if K % 4 else []) and c.wrong[4] == ([4 * (K // 4) - 1] if K >= 4 else [])
        kind, shift = c.path(5)
        assert c.wrong[5] == ([1024 - 4 * shift] if K > 1024 - 4 * shift else [])
    assert seen == {"same", "aligned", "scalar"}


def test_geometries_reach_the_paths_they_name():
    shifts_seen, second_trip_by_shift = set(), set()
    for K in CC.KS:
        for tag, d_off, t_off, ld_d, ld_t in CC.geometries(K):
            c = CC.Case(d_off, t_off, ld_d, ld_t, CC.N_ROWS, K)
            paths = [c.path(i) for i in range(c.n)]
            if tag.startswith("same shift"):
                assert paths == [("same", d_off // 4)] * c.n, tag
            elif tag.startswith("same, shift cycles"):
                assert all(p[0] == "same" for p in paths), tag
                assert len({p[1] for p in paths}) > 1 or ld_d % 32 == 0 and K == 1020, tag  # (1020 + 36 floats are 33 lines)
            elif tag.startswith("aligned at"):
                assert paths == [("aligned", 0)] * c.n, tag
            elif tag.startswith("aligned, strides"):
                assert paths[0][0] == "same" and any(p[0] == "aligned" for p in paths), tag
            else:
                assert paths == [("scalar", 0)] * c.n, tag
            for kind, shift in paths:
                if kind == "same":
                    shifts_seen.add(shift)
                    K4 = K // 4
                    if (K4 + 255) // 256 < (K4 + shift + 255) // 256:
                        second_trip_by_shift.add((K, shift))
    assert shifts_seen == set(range(8))
    # the loop bound K4 + shift takes another trip of 256 float4s because of the shift alone ...
    assert {(1000, 7), (1001, 7), (1003, 7), (1020, 2), (1020, 7)} <= second_trip_by_shift, sorted(second_trip_by_shift)
    # ... and lands exactly on a trip's end (256, 512), where it must not
    assert not {(996, 7), (1020, 1), (2020, 7)} & second_trip_by_shift and {996 // 4 + 7, 1020 // 4 + 1, 2020 // 4 + 7} == {256, 512}


def test_big_case_and_row_lists(oracle):
    c = CC.big_case()
    assert c.n == 2 * 8192 + 5 and c.K == 4 and {c.path(i)[0] for i in (0, 1, 2, 3)} == {"same"}
    dec, tx = np.ascontiguousarray(c.dec), np.ascontiguousarray(c.tx)
    assert c.expected() == oracle.count_errors(dec, tx).tolist() == [9, 4 * c.n, 5, c.n]
    assert np.flatnonzero(c.errors).tolist() == [0, 8191, 8192, 16383, 16388]
    rows = np.concatenate([np.random.RandomState(3).permutation(c.n), [0, 8192, 16388, 0]])
    assert c.expected(rows) == oracle.count_errors(dec, tx, rows).tolist() == [9 + 1 + 2 + 1 + 1, 4 * (c.n + 4), 9, c.n + 4]
    assert c.expected(rows, start=(5, 6, 7, 8)) == [19, 4 * (c.n + 4) + 6, 16, c.n + 12]


def test_value_pairs_follow_long_then_compare(oracle):
    dec, tx, wrong = CC.value_matrix()
    truth = (torch.from_numpy(dec).long() != torch.from_numpy(tx).long()).numpy()
    assert np.array_equal(truth, wrong), "the table's verdicts are torch's .long() compare"
    assert oracle.count_errors(dec, tx).tolist() == [int(wrong.sum()), wrong.size, int(wrong.any(axis=1).sum()), wrong.shape[0]]
    assert np.all(np.isfinite(dec)) and np.all(np.isfinite(tx)) and max(np.abs(dec).max(), np.abs(tx).max()) < 2.0 ** 62
    for i in range(wrong.shape[0]):  # every pair at every position of a row
        assert np.flatnonzero(wrong[:, i]).tolist() == sorted(((i - np.flatnonzero(wrong[0])) % wrong.shape[0]).tolist())


# ------------------------------------------------------------ the GPU comparisons would flag a wrong kernel
def test_the_cases_flag_wrong_counters():
    """Each mutant counts as a wrong kernel would, on the host, over the cases' own buffers: the comparison with expected() fails."""
    def count(c, lo_of, hi_of, cast=np.int64):
        """Counters of the rows when row i is read from lo_of(i) floats in front of its start to hi_of(i) floats behind its end."""
        e = []
        for i in range(c.n):
            d0, t0 = c.start["dec"] + i * c.ld["dec"], c.start["tx"] + i * c.ld["tx"]
            lo, hi = lo_of(i), c.K + hi_of(i)
            e.append(int(np.count_nonzero(c.dec_buf[d0 - lo:d0 + hi].astype(cast) != c.tx_buf[t0 - lo:t0 + hi].astype(cast))))
        e = np.array(e)
        return [int(e.sum()), c.n * c.K, int(np.count_nonzero(e)), c.n]

    flagged = {"mask": 0, "trip": 0, "tail": 0}
    total = shifted = 0
    for K in CC.KS:
        for tag, d_off, t_off, ld_d, ld_t in CC.geometries(K):
            c = CC.Case(d_off, t_off, ld_d, ld_t, CC.N_ROWS, K)
            assert count(c, lambda i: 0, lambda i: 0) == c.expected()
            if not tag.startswith("same"):
                continue
            total += 1
            shifted += any(c.path(i)[1] for i in range(c.n))
            # the shift mask dropped: the floats between the line boundary and the row are counted
            flagged["mask"] += count(c, lambda i: 4 * c.path(i)[1], lambda i: 0) != c.expected()
            # the upper bound without the shift: the last `shift` float4s of the row are not read
            flagged["trip"] += count(c, lambda i: 0, lambda i: -min(4 * c.path(i)[1], 4 * (c.K // 4))) != c.expected()
            # the tail read as a whole float4: up to three floats behind the row are counted
            flagged["tail"] += count(c, lambda i: 0, lambda i: (-c.K) % 4) != c.expected()
    print(f"of {total} same-offset geometries: {flagged}")
    assert flagged["mask"] == shifted  # every geometry with a non-zero shift in some row
    assert flagged["trip"] > total // 2 and flagged["tail"] == 16 * sum(1 for K in CC.KS if K % 4)

    # a 32-bit (saturating) cast, or a float compare, in place of the 64-bit one
    dec, tx, wrong = CC.value_matrix()
    sat32 = lambda a: np.clip(np.trunc(a.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)  # noqa: E731
    assert int((sat32(dec) != sat32(tx)).sum()) == int(wrong.sum()) - 2 * wrong.shape[0]
    assert int((dec != tx).sum()) == int(wrong.sum()) + 3 * wrong.shape[0]
