"""mvn_count_errors (count_errors_kernel) through mvn.count_errors on the cases of count_cases.py: rows placed at chosen offsets inside a
128-byte line, so that each of the kernel's read paths -- float4 loads from the line boundary below the row with the lanes in front
masked (every shift 1 .. 7), float4 loads from the row, scalar loads -- runs at every word length around its loop edges, with every
float outside the rows a mismatch that a leaking read would count.  Each geometry is counted once over all rows and once row by row,
so that a failure names the pattern.  Then the grid-stride loop's second and third pass with row lists, and the values at which
`.long()` then compare differs from a float or a 32-bit compare."""
import numpy as np
import pytest
import torch

import count_cases as CC
import meta_viterbinet_amd as mvn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def on_device(case, dev):
    """The case's two buffers at 128-byte-aligned device addresses and its [n, K] row views into them."""
    views = []
    for which, buf in (("dec", case.dec_buf), ("tx", case.tx_buf)):
        raw = torch.empty(buf.size + 32, dtype=torch.float32, device=dev)
        skip = (-raw.data_ptr() % 128) // 4
        flat = raw[skip:skip + buf.size]
        assert flat.data_ptr() % 128 == 0
        flat.copy_(torch.from_numpy(buf))
        v = torch.as_strided(flat, (case.n, case.K), (case.ld[which], 1), case.start[which])
        assert v.stride(-1) == 1 and v.stride(0) == case.ld[which]
        for i in range(case.n) if case.n <= CC.N_ROWS else (0, 1, case.n - 1):  # the geometry the case claims, from the addresses
            assert v[i].data_ptr() % 128 == case.row_mod128(which, i), (which, i)
        views.append(v)
    return views


@pytest.mark.parametrize("K", CC.KS)
def test_rows_at_chosen_offsets(dev, K):
    for tag, d_off, t_off, ld_d, ld_t in CC.geometries(K):
        case = CC.Case(d_off, t_off, ld_d, ld_t, CC.N_ROWS, K)
        dec, tx = on_device(case, dev)
        assert torch.equal(dec.cpu(), torch.from_numpy(np.ascontiguousarray(case.dec)))  # the views are the case's rows
        got = mvn.count_errors(dec, tx).tolist()
        each = torch.zeros(case.n, 4, dtype=torch.int64, device=dev)
        for i in range(case.n):
            mvn.count_errors(dec, tx, torch.tensor([i], device=dev), each[i])
        each = each.tolist()
        for i in range(case.n):
            kind, shift = case.path(i)
            assert each[i] == case.expected([i]), \
                f"K {K}, {tag}: row {i} ({CC.PATTERNS[i % 8]}, wrong at {case.wrong[i][:8]}, path {kind}, shift {shift}) counted {each[i]}"
        assert got == case.expected(), f"K {K}, {tag}"


def test_row_lists_and_the_grid_stride_loop(dev):
    """2 * 8192 + 5 rows: a launch covers 8192 rows a pass, the errors sit in the first and last row of each pass."""
    case = CC.big_case()
    dec, tx = on_device(case, dev)
    assert mvn.count_errors(dec, tx).tolist() == case.expected() == [9, 4 * case.n, 5, case.n]
    perm = np.random.RandomState(3).permutation(case.n)
    assert mvn.count_errors(dec, tx, torch.from_numpy(perm).to(dev)).tolist() == case.expected(perm)
    dup = np.concatenate([perm, [0, CC.PASS_ROWS, 2 * CC.PASS_ROWS + 4, 0]])  # a repeated row counts each time, in every counter
    assert mvn.count_errors(dec, tx, torch.from_numpy(dup).to(dev)).tolist() == case.expected(dup) == [14, 4 * (case.n + 4), 9, case.n + 4]
    for rows in ([CC.PASS_ROWS - 1], [CC.PASS_ROWS], [2 * CC.PASS_ROWS + 4, 2 * CC.PASS_ROWS + 4], [1, 2, 3]):
        assert mvn.count_errors(dec, tx, torch.tensor(rows, device=dev)).tolist() == case.expected(rows), rows
    start = torch.tensor([5, 6, 7, 8], dtype=torch.int64, device=dev)  # accumulates into what the counters hold
    out = mvn.count_errors(dec, tx, torch.from_numpy(dup).to(dev), start)
    assert out is start and out.tolist() == case.expected(dup, start=(5, 6, 7, 8))


def test_values_are_compared_as_int64(dev):
    """`.long()` then compare: truth is torch's own on the CPU.  The pairs tell a float compare ((0.9, 0.2): both 0) and a 32-bit or
    saturating cast (3000000000 against 3000000256, 2^40 against 2^40 + 2^17) from it.  Finite values below 2^62 only: a non-finite
    or larger float casts differently on host and device, and the detectors never produce one."""
    dec, tx, _ = CC.value_matrix()
    truth = (torch.from_numpy(dec).long() != torch.from_numpy(tx).long()).numpy()
    n = dec.shape[0]
    want = [int(truth.sum()), truth.size, int(truth.any(axis=1).sum()), n]
    for pad in (0, 1):  # rows 16-byte aligned (float4 loads and a scalar tail) and not (scalar loads)
        d = torch.zeros(n, 12 + pad, device=dev)[:, :n]
        t = torch.zeros(n, 12 + pad, device=dev)[:, :n]
        d.copy_(torch.from_numpy(dec))
        t.copy_(torch.from_numpy(tx))
        assert mvn.count_errors(d, t).tolist() == want, pad
        for i in range(n):
            assert mvn.count_errors(d, t, torch.tensor([i], device=dev)).tolist() == [int(truth[i].sum()), n, int(truth[i].any()), 1], (pad, i)
    for p, t, wrong in CC.VALUE_PAIRS:  # each pair alone names itself
        got = mvn.count_errors(torch.tensor([[p]], device=dev), torch.tensor([[t]], device=dev)).tolist()
        assert got == [wrong, 1, wrong, 1], (p, t)
