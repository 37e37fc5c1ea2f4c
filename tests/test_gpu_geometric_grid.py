"""gpu tier: tkmk_poly_geometric_grid (csrc/poly.hip) — out[i][k] = c0 * gx^i * gy^(col0 + col_step k), written with no input array —
against Python integers.  Exact equality: this is integer arithmetic, there is no tolerance.

Shapes: one element; a few rows and columns; a sharded rank's column slice (col0 = 3, col_step = 4); more rows than one 256-thread
block covers; a row wider than one block and than any per-thread run, with a row boundary inside a block.  Generator cases: random
gx, gy; gx = 1; gy = 0 from column 0 (0^0 = 1: column 0 is c0 gx^i, the rest 0); gx = w_8 with 17 rows (the exponent wraps the
order).  Every case once with a random c0 and once with c0 = 1."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SHAPES = [(1, 1, 0, 1), (3, 5, 0, 1), (5, 3, 3, 4), (257, 3, 1, 2), (2, 1025, 0, 1)]


def _fr(v):
    return np.frombuffer(int(v % R).to_bytes(32, "little"), np.uint8).copy()


def _expected(rows, cols, c0, gx, gy, col0, col_step):
    ys = [pow(gy, col0 + col_step * k, R) for k in range(cols)]            # Python: pow(0, 0, R) == 1
    out, xi = [], c0 % R
    for _ in range(rows):
        out.extend(xi * y % R for y in ys)
        xi = xi * gx % R
    return out


def _run(gpu, rows, cols, c0, gx, gy, col0, col_step):
    buf = gpu.poly_geometric_grid(rows, cols, _fr(c0), _fr(gx), _fr(gy), col0, col_step)
    raw = buf.to_host().tobytes()
    assert len(raw) == 32 * rows * cols
    got = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    want = _expected(rows, cols, c0, gx, gy, col0, col_step)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "first mismatch at element %d (row %d, local column %d) of %d" % (bad[0], bad[0] // cols, bad[0] % cols, len(bad))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("unit_c0", [False, True], ids=["c0_random", "c0_one"])
def test_random_generators(gpu, shape, unit_c0):
    rng = random.Random(hash(shape) & 0xFFFF)
    c0 = 1 if unit_c0 else rng.randrange(1, R)
    _run(gpu, shape[0], shape[1], c0, rng.randrange(2, R), rng.randrange(2, R), shape[2], shape[3])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("unit_c0", [False, True], ids=["c0_random", "c0_one"])
def test_gx_one(gpu, shape, unit_c0):
    rng = random.Random(101 + shape[0])
    c0 = 1 if unit_c0 else rng.randrange(1, R)
    _run(gpu, shape[0], shape[1], c0, 1, rng.randrange(2, R), shape[2], shape[3])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] == 0], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("unit_c0", [False, True], ids=["c0_random", "c0_one"])
def test_gy_zero_from_column_zero(gpu, shape, unit_c0):
    rng = random.Random(202 + shape[1])
    c0 = 1 if unit_c0 else rng.randrange(1, R)
    _run(gpu, shape[0], shape[1], c0, rng.randrange(2, R), 0, 0, shape[3])


@pytest.mark.parametrize("unit_c0", [False, True], ids=["c0_random", "c0_one"])
def test_gx_of_order_eight_wraps_over_seventeen_rows(gpu, unit_c0):
    w8 = int.from_bytes(bytes(gpu.get_root_of_unity_with_generator(5, 8)), "little")
    assert pow(w8, 8, R) == 1 and pow(w8, 4, R) == R - 1
    rng = random.Random(303)
    c0 = 1 if unit_c0 else rng.randrange(1, R)
    _run(gpu, 17, 5, c0, w8, rng.randrange(2, R), 0, 1)


def test_arguments_are_checked(gpu):
    one = _fr(1)
    out = gpu.DeviceBuffer(32)
    for rows, cols, col0, step in ((0, 1, 0, 1), (1, 0, 0, 1), (1, 3, (1 << 32) - 2, 1), (1, 3, 0, 1 << 31)):
        with pytest.raises(gpu.TkmkError) as e:
            gpu.poly_geometric_grid(rows, cols, one, one, one, col0, step, out=out)
        assert e.value.code == 11, (rows, cols, col0, step)
