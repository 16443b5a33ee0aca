"""Cases for mvn_count_errors (count_errors_kernel) at chosen row geometries: where the two rows sit inside a 128-byte line decides
which of the kernel's three read paths runs -- float4 loads issued from the line boundary below the row with the lanes in front of
it masked (both rows 16-byte aligned at the SAME offset `shift` float4s into a line), float4 loads from the row start (aligned at
different offsets), scalar loads (either row unaligned) -- and K decides the trips of 256 float4s and the scalar tail.

A case is two flat float32 buffers whose first element stands for a 128-byte-aligned address, the strided row views into them, and
the counters the rows must give.  Every float OUTSIDE the rows is a guaranteed mismatch (1.0 in dec, 0.0 in tx): 32 floats in front
of the first row, the gaps between rows, at least 32 floats behind the last -- a read that leaks past a row changes the count.

tests/test_count_cases_host.py checks the builder against the CPU oracle; tests/test_gpu_count_errors.py runs the kernel on it."""
import numpy as np

FRONT = 32  # floats (one 128-byte line) of mismatching fill in front of the first row and behind the last
KS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 993, 996, 1000, 1001, 1003, 1020, 1024, 1028, 2017, 2020, 2052)
N_ROWS = 8
PATTERNS = ("clean", "first", "last", "tail_first", "tail_before", "second_trip", "all", "random")


def up(k, m):
    return (k + m - 1) // m * m


def shift_of(off):
    """float4s between the 128-byte line boundary below float offset `off` (from an aligned base) and `off`."""
    return (4 * off % 128) // 16


def pattern_positions(pattern, K, shift, rng):
    """The positions in a row of K symbols that the pattern makes wrong ([] where the pattern's element does not exist at this K)."""
    K4 = 4 * (K // 4)
    pos = {"clean": [], "first": [0], "last": [K - 1], "tail_first": [K4] if K4 < K else [], "tail_before": [K4 - 1] if K4 else [],
           "second_trip": [1024 - 4 * shift] if K > 1024 - 4 * shift else [], "all": list(range(K)),
           "random": np.flatnonzero(rng.rand(K) < 0.01).tolist()}[pattern]
    return sorted(set(pos))


class Case:
    """dec_buf / tx_buf: the flat buffers; dec / tx: their [n, K] row views; off / ld: the rows' geometry in floats from the aligned
    base (FRONT floats into the buffer); wrong: per row, the planted positions; errors: int64 [n], the wrong symbols of each row."""

    def __init__(self, dec_off, tx_off, ld_dec, ld_tx, n, K, plan=None, seed=0):
        assert ld_dec >= K and ld_tx >= K and n >= 1 and K >= 1 and dec_off >= 0 and tx_off >= 0
        rng = np.random.RandomState(seed + 7919 * K + dec_off + 31 * tx_off)
        self.n, self.K = n, K
        self.off = {"dec": dec_off, "tx": tx_off}
        self.ld = {"dec": ld_dec, "tx": ld_tx}
        self.start = {"dec": FRONT + dec_off, "tx": FRONT + tx_off}  # of row 0 in the flat buffers
        self.dec_buf = np.full(up(self.start["dec"] + (n - 1) * ld_dec + K + FRONT, 32), 1.0, np.float32)
        self.tx_buf = np.full(up(self.start["tx"] + (n - 1) * ld_tx + K + FRONT, 32), 0.0, np.float32)
        self.dec, self.tx = self.views(self.dec_buf, self.tx_buf)
        words = rng.randint(0, 2, (n, K)).astype(np.float32)
        self.tx[:] = words
        self.dec[:] = words
        self.wrong = []
        for i in range(n):
            if plan is None:
                pos = pattern_positions(PATTERNS[i % len(PATTERNS)], K, self.path(i)[1], rng)
            else:
                pos = sorted(plan.get(i, []))
            self.dec[i, pos] = 1.0 - self.dec[i, pos]
            self.wrong.append(pos)
        self.errors = np.array([len(p) for p in self.wrong], np.int64)

    def views(self, dec_buf, tx_buf):
        """The [n, K] row views (row stride ld, last stride 1) into buffers laid out like dec_buf / tx_buf."""
        st = np.lib.stride_tricks.as_strided
        return (st(dec_buf[self.start["dec"]:], (self.n, self.K), (4 * self.ld["dec"], 4)),
                st(tx_buf[self.start["tx"]:], (self.n, self.K), (4 * self.ld["tx"], 4)))

    def row_mod128(self, which, i):
        """Byte offset of row i inside its 128-byte line, given an aligned base."""
        return 4 * (self.off[which] + i * self.ld[which]) % 128

    def path(self, i):
        """The kernel's read path for row i: 'same' (with its shift), 'aligned' or 'scalar'."""
        d, t = self.row_mod128("dec", i), self.row_mod128("tx", i)
        if d % 16 or t % 16:
            return ("scalar", 0)
        return ("same", d // 16) if d == t else ("aligned", 0)

    def expected(self, rows=None, start=(0, 0, 0, 0)):
        """[bit errors, bits, frame errors, frames] over `rows` (default all; a repeated row counts each time) added to `start`."""
        e = self.errors if rows is None else self.errors[np.asarray(rows, np.int64)]
        return [int(start[0] + e.sum()), int(start[1] + e.size * self.K), int(start[2] + np.count_nonzero(e)), int(start[3] + e.size)]


def geometries(K):
    """(tag, dec_off, tx_off, ld_dec, ld_tx) at word length K."""
    line, cyc = up(K, 32) + 32, up(K, 4) + 36  # rows a whole number of lines apart: one shift; 36 floats more than K: the shift cycles
    out = []
    for off in range(0, 32, 4):
        out.append((f"same shift {off // 4}", off, off, line, line))
        out.append((f"same, shift cycles from {off // 4}", off, off, cyc, cyc))
    for d, t in ((0, 4), (4, 0), (8, 28), (12, 16)):
        out.append((f"aligned at {d} / {t}", d, t, line, line))
    out.append(("aligned, strides differ", 8, 8, line, line + 4))  # the same offset in row 0 only (and every eighth row)
    for o in (1, 2, 3):
        out.append((f"dec unaligned by {o}", o, 0, cyc, cyc))
        out.append((f"tx unaligned by {o}", 4, 4 + o, cyc, cyc))
        out.append((f"both unaligned by {o}", 8 + o, 8 + o, cyc, cyc))
    return out


# the grid-stride loop: one launch is 512 workgroups of 16 waves, one wave per row -- 8192 rows a pass
PASS_ROWS = 8192
BIG_N, BIG_K = 2 * PASS_ROWS + 5, 4
BIG_PLAN = {0: [0], PASS_ROWS - 1: [3], PASS_ROWS: [1, 2], 2 * PASS_ROWS - 1: [0, 1, 2, 3], 2 * PASS_ROWS + 4: [2]}


def big_case():
    return Case(4, 4, 8, 8, BIG_N, BIG_K, plan=BIG_PLAN)


# .long() then compare (metrics.py:7-17): pairs (prediction, target) and whether they count as an error -- truncation toward zero in
# 64 bits.  A float compare gets (0.9, 0.2), (1.0, 1.9), (-0.5, 0.0) wrong, a 32-bit (saturating) cast the last two.  Finite values
# below 2^62 only: a non-finite or larger float casts differently on host and device, and no detector produces one.
VALUE_PAIRS = ((0.0, -0.0, 0), (0.9, 0.2, 0), (1.0, 1.9, 0), (1.0, 2.0, 1), (-0.5, 0.0, 0), (-1.0, 1.0, 1), (0.99999994, 1.0, 1),
               (3000000000.0, 3000000256.0, 1), (2.0 ** 40, 2.0 ** 40 + 2.0 ** 17, 1))


def value_matrix():
    """(dec, tx, wrong): [9, 9] float32 each, row i the pairs rotated by i -- every pair at every position of a row (the float4 part
    and the scalar tail) -- and the bool matrix of the pairs that count."""
    p = np.array([v[0] for v in VALUE_PAIRS], np.float32)
    t = np.array([v[1] for v in VALUE_PAIRS], np.float32)
    w = np.array([v[2] for v in VALUE_PAIRS], bool)
    n = len(VALUE_PAIRS)
    return (np.stack([np.roll(p, i) for i in range(n)]), np.stack([np.roll(t, i) for i in range(n)]),
            np.stack([np.roll(w, i) for i in range(n)]))
