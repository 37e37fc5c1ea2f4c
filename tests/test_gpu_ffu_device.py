"""gpu tier: the device's unsaturated products (csrc/ffu.h: the generated column chains of field_params.h) through tkmk_diag_ffu, limb for
limb against the big-integer definition of the result (tests/ffu_ref.py, itself checked against the host build by
tests/test_ffu_reference.py).  Both fields; one launch of about 2000 lanes per op and field."""
import ctypes

import numpy as np
import pytest

import ffu_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("curve", sorted(ffu_ref.FIELDS))
@pytest.mark.parametrize("op", ffu_ref.OPS, ids=[ffu_ref.OP_NAMES[o] for o in ffu_ref.OPS])
def test_device_ffu_equals_the_reference_limb_for_limb(gpu, curve, op):
    (a, b, c, d), want = ffu_ref.operand_set(curve, op)
    assert gpu.FFU_LIMBS[curve] == (ffu_ref.FIELDS[curve]["L"], ffu_ref.FIELDS[curve]["W"])
    got = gpu.diag_ffu(curve, op, a, b, c, d)
    assert got.shape == want.shape and want.shape[0] >= ffu_ref.RANDOM_TUPLES
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:1]], want[bad[:1]])


def test_diag_ffu_refuses_what_it_cannot_run(gpu):
    (a, b, _, _), _ = ffu_ref.operand_set(0, ffu_ref.MUL)
    with pytest.raises(ValueError):
        gpu.diag_ffu(0, ffu_ref.MUL_ADD, a, b)                 # mul_add reads four operands
    with pytest.raises(ValueError):
        gpu.diag_ffu(1, ffu_ref.MUL, a, b)                     # 14-limb operands for the 10-limb field
    one = ctypes.c_uint64(1)
    assert gpu.lib().tkmk_diag_ffu(2, 0, None, None, None, None, None, one) == 11        # no such curve: TKMK_ERR_INVALID_ARGUMENT
    assert gpu.lib().tkmk_diag_ffu(0, 4, None, None, None, None, None, one) == 11        # no such op
    assert gpu.lib().tkmk_diag_ffu(0, 0, None, None, None, None, None, one) == 3         # TKMK_ERR_INVALID_POINTER
