"""not-gpu tier: the big-integer definition of ffu's products (tests/ffu_ref.py) against the HOST build of csrc/ffu.h with every FFU_ASSERT
live (tests/hostcheck/hostcheck_ffu_raw.cpp), limb for limb, on the operand set the device check uses (tests/test_gpu_ffu_device.py).
This validates the reference — and that the operand set keeps every bound of ffu.h: a violated one aborts the process — without a GPU."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import ffu_ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hf():
    spec = importlib.util.spec_from_file_location("hostcheck_build_ffu_raw", os.path.join(HERE, "hostcheck", "build_ffu_raw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = mod.build()
    assert so is not None, "hipcc is needed to compile the host check"
    return ctypes.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_reference_is_the_montgomery_product_mod_p():
    """the exact definition is a Montgomery product: r R = a b + c d (mod p), and r < 1.03 p for operands within a b + c d < 2^20 p^2"""
    for curve, f in ffu_ref.FIELDS.items():
        p, L, W = f["p"], f["L"], f["W"]
        R = 1 << (W * L)
        for op in ffu_ref.OPS:
            ops, want = ffu_ref.operand_set(curve, op)
            for i in range(0, want.shape[0], 7):
                v = [ffu_ref.value(x[i], W) for x in ops if x is not None]
                t = v[0] * v[0] if op == ffu_ref.SQR else v[0] * v[1] + (v[2] * v[3] if len(v) == 4 else 0)
                r = ffu_ref.value(want[i], W)
                assert (r * R - t) % p == 0 and 100 * r < 103 * p
                assert all(int(x) < (1 << W) for x in want[i][:-1])


@pytest.mark.parametrize("curve", sorted(ffu_ref.FIELDS))
@pytest.mark.parametrize("op", ffu_ref.OPS, ids=[ffu_ref.OP_NAMES[o] for o in ffu_ref.OPS])
def test_host_ffu_equals_the_reference_limb_for_limb(hf, curve, op):
    ops, want = ffu_ref.operand_set(curve, op)
    n, L = want.shape
    assert L == ffu_ref.FIELDS[curve]["L"] and n >= ffu_ref.RANDOM_TUPLES
    out = np.zeros((n, L), np.uint32)
    assert hf.hc_ffu_raw(curve, op, _p(ops[0]), _p(ops[1]), _p(ops[2]), _p(ops[3]), _p(out), ctypes.c_size_t(n)) == 0
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], out[bad[:1]], want[bad[:1]])


def test_operand_set_holds_the_edges_the_curve_formulas_reach():
    """0, 1, the Montgomery one, p - 1, p, p + 1, 2p - 1, the accumulator (5.03 p) and P (9.03 p) bounds of ec_u.h, the fullest columns
    below 2^10 p; for mul_add<true> a c with every lower limb 2^(W+1) - 1"""
    for curve, f in ffu_ref.FIELDS.items():
        p, L, W = f["p"], f["L"], f["W"]
        e = ffu_ref.edge_values(curve)
        assert len(e) == 10 and e[:2] == [0, 1] and e[2] == pow(2, W * L, p) and e[3:7] == [p - 1, p, p + 1, 2 * p - 1]
        assert 0 < 503 * p - 100 * e[7] <= 200 and 0 < 903 * p - 100 * e[8] <= 200 and e[9] < (1 << 10) * p <= e[9] + (1 << (W * (L - 1)))
        (a, b, _, _), _ = ffu_ref.operand_set(curve, ffu_ref.MUL)
        pairs = {(ffu_ref.value(x, W), ffu_ref.value(y, W)) for x, y in zip(a[:100], b[:100])}
        assert pairs == {(x, y) for x in e for y in e}
        (_, _, c, _), _ = ffu_ref.operand_set(curve, ffu_ref.MUL_ADD_UNSWEPT)
        full = [(1 << (W + 1)) - 1] * (L - 1)
        tops = [int(r[-1]) for r in c if list(r[:-1]) == full]
        assert tops and max(tops) <= 25 and (curve != 0 or max(tops) == 25)
        assert int(c.max()) < (1 << (W + 1))
