"""gpu tier: the two kernels of the witness check (csrc/witcheck.hip: tkmk_witness_check_r1cs, tkmk_witness_check_copy) against Python
integers mod r.  The shapes are the smallest at which the r1cs kernel's tiling can go wrong: one cell, a padded stride, exactly one wave
per row, both tile boundaries crossed (64 columns per workgroup, 64 rows per chunk, four waves a chunk), many rows under fewer columns
than a wave.  Both results are a count and a minimum over integers, so every call is made twice and must repeat itself bit for bit."""
import random

import numpy as np
import pytest

from pyref import R

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
SHAPES = [(1, 1, 1), (3, 5, 8), (64, 64, 64), (65, 130, 130), (4096, 3, 3)]   # rows, cols, stride


def _bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), np.uint8)


class Grid:
    """u, v random with the edge values 0, 1, r - 1 mixed in, w = u v mod r; padding columns hold cells that FAIL"""

    def __init__(self, tk, rows, cols, stride, seed):
        rnd = random.Random(seed)
        self.tk, self.rows, self.cols, self.stride = tk, rows, cols, stride
        pick = lambda: rnd.choice((0, 1, R - 1)) if rnd.random() < 0.1 else rnd.randrange(R)      # noqa: E731
        self.u = [pick() for _ in range(rows * stride)]
        self.v = [pick() for _ in range(rows * stride)]
        self.w = [a * b % R for a, b in zip(self.u, self.v)]
        for r in range(rows):
            for c in range(cols, stride):
                self.w[r * stride + c] = (self.w[r * stride + c] + 1) % R
        self.d_u, self.d_v = tk.DeviceBuffer.from_host(_bytes(self.u)), tk.DeviceBuffer.from_host(_bytes(self.v))

    def expect(self, u, v, w):
        cnt, first = np.zeros(self.cols, np.uint32), np.full(self.cols, NONE, np.uint32)
        for r in range(self.rows):
            for c in range(self.cols):
                at = r * self.stride + c
                if u[at] * v[at] % R != w[at]:
                    cnt[c] += 1
                    first[c] = min(first[c], r)
        return cnt, first

    def check(self, w, u=None, v=None):
        tk = self.tk
        d_u = self.d_u if u is None else tk.DeviceBuffer.from_host(_bytes(u))
        d_v = self.d_v if v is None else tk.DeviceBuffer.from_host(_bytes(v))
        w_bytes = _bytes(w)
        d_w = tk.DeviceBuffer.from_host(w_bytes)
        want_cnt, want_first = self.expect(self.u if u is None else u, self.v if v is None else v, w)
        got = tk.witness_check_r1cs(d_u, d_v, d_w, self.rows, self.cols, self.stride)
        again = tk.witness_check_r1cs(d_u, d_v, d_w, self.rows, self.cols, self.stride)
        assert (got[0] == want_cnt).all() and (got[1] == want_first).all(), (got, want_cnt, want_first)
        assert got[2] == int(want_cnt.sum())
        assert (got[0] == again[0]).all() and (got[1] == again[1]).all() and got[2] == again[2]      # order-independent: identical from run to run
        assert (d_w.to_host() == w_bytes).all()                                                       # the grid is read, never written
        return got


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d_stride%d" % s)
def grid(gpu, request):
    rows, cols, stride = request.param
    return Grid(gpu, rows, cols, stride, seed=1000 + rows + cols)


def test_all_cells_good(grid):
    cnt, first, total = grid.check(grid.w)
    assert total == 0 and not cnt.any() and (first == NONE).all()


@pytest.mark.parametrize("where", ["first", "last", "random"])
def test_exactly_one_bad_cell(grid, where):
    rnd = random.Random(7)
    r, c = {"first": (0, 0), "last": (grid.rows - 1, grid.cols - 1), "random": (rnd.randrange(grid.rows), rnd.randrange(grid.cols))}[where]
    w = list(grid.w)
    w[r * grid.stride + c] = (w[r * grid.stride + c] + 1) % R
    cnt, first, total = grid.check(w)
    assert total == 1 and cnt[c] == 1 and first[c] == r


def test_every_cell_bad(grid):
    w = [(x + 1) % R for x in grid.w]
    cnt, first, total = grid.check(w)
    assert (cnt == grid.rows).all() and (first == 0).all() and total == grid.rows * grid.cols


def test_column_failing_in_its_last_row_only(grid):
    c = grid.cols // 2
    w = list(grid.w)
    w[(grid.rows - 1) * grid.stride + c] = (w[(grid.rows - 1) * grid.stride + c] + 5) % R
    cnt, first, total = grid.check(w)
    assert total == 1 and cnt[c] == 1 and first[c] == grid.rows - 1


def test_edge_values_and_the_product_mod_2_256(grid):
    """u = v = r - 1, w = 1 holds; w = (u v mod 2^256) reduced into range is NOT u v mod r wherever the two differ: a multiplier that
    drops the high half of the product, or skips the reduction, passes the one and fails the other"""
    rnd = random.Random(11)
    u, v, w = list(grid.u), list(grid.v), list(grid.w)
    cells = [(r, c) for r in range(grid.rows) for c in range(grid.cols)]
    rnd.shuffle(cells)
    wrapped = 0
    for k, (r, c) in enumerate(cells[:64]):
        at = r * grid.stride + c
        if k % 2 == 0:
            u[at], v[at], w[at] = R - 1, R - 1, 1
        else:
            u[at], v[at] = rnd.randrange(R >> 1, R), rnd.randrange(R >> 1, R)
            w[at] = (u[at] * v[at] % (1 << 256)) % R
            wrapped += w[at] != u[at] * v[at] % R
    cnt, first, total = grid.check(w, u, v)
    assert total == wrapped
    assert wrapped > 0 or len(cells) < 2


def test_padding_of_the_outputs_is_not_written(gpu):
    """3 x 5 in a stride of 8: the failing padding cells take no part, and entries n_cols.. of the two output arrays keep their bytes"""
    g = Grid(gpu, 3, 5, 8, seed=3)
    sentinel = np.full(8, 0xA5A5A5A5, np.uint32)
    outs = (gpu.DeviceBuffer.from_host(sentinel.view(np.uint8)), gpu.DeviceBuffer.from_host(sentinel.view(np.uint8)))
    cnt, first, total = gpu.witness_check_r1cs(g.d_u, g.d_v, gpu.DeviceBuffer.from_host(_bytes(g.w)), 3, 5, 8, outs=outs)
    assert total == 0 and not cnt.any() and (first == NONE).all()
    for o in outs:
        assert (o.to_host().view(np.uint32)[5:] == sentinel[5:]).all()
    with pytest.raises(gpu.TkmkError) as e:
        gpu.witness_check_r1cs(g.d_u, g.d_v, g.d_u, 3, 9, 8)              # n_cols > stride
    assert e.value.code == 11


# ------------------------------------------------------------------------------------------------------------------ the copy kernel
class CopyGrid:
    def __init__(self, tk, rows, cols, stride, seed):
        rnd = random.Random(seed)
        pool = [rnd.randrange(R) for _ in range(3)] + [0]
        self.rows, self.cols, self.stride, self.rnd = rows, cols, stride, rnd
        self.b = [rnd.choice(pool) for _ in range(rows * stride)]
        self.d_b = tk.DeviceBuffer.from_host(_bytes(self.b))
        cells = [(r, c) for r in range(rows) for c in range(cols)]
        self.equal = [(r * stride + c, x, y) for r, c in cells for x, y in cells if self.b[r * stride + c] == self.b[x * stride + y]]
        self.differ = [(r * stride + c, x, y) for r, c in cells for x, y in cells if self.b[r * stride + c] != self.b[x * stride + y]]

    def run(self, tk, entries):
        cols3 = [[e[k] for e in entries] for k in range(3)]
        got = tk.witness_check_copy(self.d_b, self.rows, self.cols, self.stride, *cols3)
        assert got == tk.witness_check_copy(self.d_b, self.rows, self.cols, self.stride, *cols3)
        bad = [k for k, (d, x, y) in enumerate(entries)
               if d // self.stride < self.rows and d % self.stride < self.cols and x < self.rows and y < self.cols and self.b[d] != self.b[x * self.stride + y]]
        assert got[0] == len(bad) and got[1] == (bad[0] if bad else None)
        return got


@pytest.fixture(scope="module", params=[(6, 5, 5), (6, 5, 8)], ids=["dense", "stride_gt_cols"])
def copy_grid(gpu, request):
    return CopyGrid(gpu, *request.param, seed=21)


def test_copy_zero_entries(gpu, copy_grid):
    assert copy_grid.run(gpu, []) == (0, None, True)
    assert gpu.witness_check_copy(None, 6, 5, 5, [], [], []) == (0, None, True)


def test_copy_consistent_map(gpu, copy_grid):
    g = copy_grid
    assert g.run(gpu, [g.rnd.choice(g.equal) for _ in range(700)]) == (0, None, True)            # three workgroups


@pytest.mark.parametrize("n", [1, 64, 257, 700])
def test_copy_one_bad_entry_first_and_last(gpu, copy_grid, n):
    g = copy_grid
    good = [g.rnd.choice(g.equal) for _ in range(n)]
    wrong = g.rnd.choice(g.differ)
    assert g.run(gpu, [wrong] + good[1:]) == (1, 0, True)
    assert g.run(gpu, good[:-1] + [wrong]) == (1, n - 1, True)
    if n > 2:
        assert g.run(gpu, good[:n // 2] + [wrong] + good[n // 2 + 1:-1] + [wrong]) == (2, n // 2, True)


def test_copy_entries_outside_the_grid_are_skipped_and_reported(gpu, copy_grid):
    g = copy_grid
    good = [g.rnd.choice(g.equal) for _ in range(300)]
    wrong = g.rnd.choice(g.differ)
    past_rows = (good[0][0], g.rows, 0)                                   # X = rows
    past_grid = (g.rows * g.stride + 3, 0, 0)                             # dst behind the last row
    for outside in (past_rows, past_grid, (good[0][0], 0, g.cols)):
        entries = good[:100] + [outside] + good[100:280] + [wrong] + good[281:]
        assert g.run(gpu, entries) == (1, 281, False)                     # TKMK_ERR_INVALID_ARGUMENT, the valid entries judged
    if g.stride > g.cols:
        assert g.run(gpu, [(g.cols, 0, 0)] + good) == (0, None, False)    # a destination in the padding of row 0
