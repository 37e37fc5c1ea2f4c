"""gpu tier: tkmk_witness_check_copy and tkmk_witness_check_copy_split (csrc/witcheck.hip) are one kernel under two addressings.  The same
entries over one 6 x 5 grid, given to both — the split entry takes the whole grid as its local cells and as its gathered sources, slot =
x * stride + y — must get the same (bad, first, in_range) from both, and that is what Python integers mod r say.  Entry counts on both
sides of a wave (63, 64, 65) and of a workgroup (255, 256, 257) and into a third workgroup (700); the single failures sit on the same
edges.  The buffer is exactly rows * stride elements long and an out-of-range entry points at the first row behind it, or far behind it:
the assertions are on the return code and the counts."""
import random

import numpy as np
import pytest

from pyref import R

pytestmark = pytest.mark.gpu
ROWS, COLS = 6, 5
BOTH_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 700]


def _bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8)


class Grid:
    """6 x 5 cells of random residues at a stride, a few of them made equal to another cell (one of those in its other representation,
    v + r); the padding columns of a wider stride hold values too, and no entry of these tests points at them: the split entry has no
    notion of padding"""

    def __init__(self, tk, stride, seed):
        rnd = random.Random(seed)
        self.tk, self.rnd, self.stride = tk, rnd, stride
        self.val = [rnd.randrange(R) for _ in range(ROWS * stride)]
        cells = [(r, c) for r in range(ROWS) for c in range(COLS)]
        rnd.shuffle(cells)
        self.equal = []
        for k in range(0, 12, 2):                                                 # six deliberate pairs
            (r, c), (x, y) = cells[k], cells[k + 1]
            self.val[r * stride + c] = self.val[x * stride + y] + (R if k == 0 else 0)
            self.equal += [(r, c, x, y), (x, y, r, c)]
        self.differ = [(r, c, x, y) for r, c in cells for x, y in cells if (self.val[r * stride + c] - self.val[x * stride + y]) % R]
        assert len(self.differ) == 30 * 29 - len(self.equal) and self.val[cells[0][0] * stride + cells[0][1]] >= R
        self.d_b = tk.DeviceBuffer.from_host(_bytes(self.val))

    def good(self, n):
        return [self.rnd.choice(self.equal) for _ in range(n)]

    def wrong(self):
        return self.rnd.choice(self.differ)

    def both(self, entries):
        """-> the (bad, first, in_range) both entries gave, after it agreed with the integers"""
        tk, stride, cells = self.tk, self.stride, ROWS * self.stride
        dst, x, y = ([e[0] * stride + e[1] for e in entries], [e[2] for e in entries], [e[3] for e in entries])
        slot = [min(e[2] * stride + e[3], 0xFFFFFFFF) for e in entries]
        got = tk.witness_check_copy(self.d_b, ROWS, COLS, stride, dst, x, y)
        assert got == tk.witness_check_copy_split(self.d_b, cells, dst, self.d_b, cells, slot)
        inside = [d < cells and s < cells for d, s in zip(dst, slot)]
        assert all(e[1] < COLS and e[3] < COLS for e, ok in zip(entries, inside) if ok)      # nothing valid points into the padding
        bad = [k for k, (d, s) in enumerate(zip(dst, slot)) if inside[k] and (self.val[d] - self.val[s]) % R]
        assert got == (len(bad), bad[0] if bad else None, all(inside)), (got, bad[:4], all(inside))
        return got


@pytest.fixture(scope="module", params=[5, 8], ids=["stride5", "stride8"])
def grid(gpu, request):
    return Grid(gpu, request.param, seed=47 + request.param)


@pytest.mark.parametrize("n", BOTH_COUNTS)
def test_both_copy_entries_decide_the_same_comparison(grid, n):
    assert grid.both(grid.good(n)) == (0, None, True)
    if n == 0:
        return
    for at in sorted({0, n - 1} | {k for k in (63, 64, 255, 256) if k < n}):       # one failure: the ends, the wave and workgroup edges
        entries = grid.good(n)
        entries[at] = grid.wrong()
        assert grid.both(entries) == (1, at, True), (n, at)
    assert grid.both([grid.wrong() for _ in range(n)]) == (n, 0, True)
    # one entry outside the grid — its destination row, or its source row, is the first one behind it — among good and failing ones:
    # code 11 from both, with the same counts
    for outside in ((ROWS, 0, 0, 0), (0, 0, ROWS, 0), (0xFFFFFFFF // grid.stride, 0, 0, 0)):
        entries = grid.good(n)
        for at in {0, n - 1}:
            entries[at] = grid.wrong()
        entries[n // 2] = outside
        failing = sorted({0, n - 1} - {n // 2})
        assert grid.both(entries) == (len(failing), failing[0] if failing else None, False), (n, outside)
