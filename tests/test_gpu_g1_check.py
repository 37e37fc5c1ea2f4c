"""GPU parity tier: tkmk_g1_check (csrc/g1check.hip) against the big-integer verdict of tests/g1_torsion.py — canonical, then curve, then
[r]P = infinity — on valid points, infinity, off-curve and noncanonical records, and points outside the prime-order subgroup (every prime
order dividing the cofactor, G + T, a random curve point).  Every comparison is exact: verdict bytes, every counter, first_bad."""
import ctypes

import numpy as np
import pytest

import g1_torsion as gt

pytestmark = pytest.mark.gpu

UINT64_MAX = (1 << 64) - 1


def _split():
    good = [(x, y) for k, x, y in gt.check_inputs() if k in ("valid", "infinity")]
    bad = [(x, y) for k, x, y in gt.check_inputs() if k not in ("valid", "infinity")]
    return good, bad


def _layout(n, bad_pool):
    """n records: valid points and infinity in rotation, bad records at index 0, n - 1, on both sides of every wave boundary, and (where n
    leaves room) every bad record of the pool once; which bad record lands where rotates with n"""
    good, _ = _split()
    recs = [good[i % len(good)] for i in range(n)]
    spots = [s for s in (0, n - 1, 63, 64, 127, 128, 191, 192) if 0 <= s < n]
    spots += [s for s in range(70, 70 + len(bad_pool)) if s < n - 1]
    for k, s in enumerate(dict.fromkeys(spots)):
        recs[s] = bad_pool[(k + n) % len(bad_pool)]
    return recs


def _bytes(recs):
    return np.concatenate([gt.to_record(x, y) for x, y in recs]) if recs else np.empty(0, np.uint8)


def _expect(recs, verdicts=None):
    v = [gt.verdict(x, y) for x, y in recs] if verdicts is None else list(verdicts)
    bad = [i for i, b in enumerate(v) if b]
    rep = {"n_checked": len(recs), "n_infinity": sum(1 for x, y in recs if x == 0 and y == 0),
           "n_noncanonical": v.count(gt.BAD_NONCANONICAL), "n_off_curve": v.count(gt.BAD_OFF_CURVE),
           "n_not_in_subgroup": v.count(gt.BAD_NOT_IN_SUBGROUP), "first_bad": bad[0] if bad else UINT64_MAX}
    return rep, np.array(v, np.uint8)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_verdicts_counters_and_first_bad(gpu, n):
    _, bad = _split()
    recs = _layout(n, bad)
    want_rep, want_v = _expect(recs)
    rep, v = gpu.g1_check(_bytes(recs))
    assert (v == want_v).all(), np.nonzero(v != want_v)[0]
    assert rep == want_rep
    if n:
        assert set(want_v.tolist()) - {0}, "the layout holds bad records"
    rep2, v2 = gpu.g1_check(_bytes(recs), want_verdicts=False)          # verdict_dev = NULL: the same report
    assert v2 is None and rep2 == want_rep


def test_every_kind_alone_and_a_clean_table(gpu):
    for kind, x, y in gt.check_inputs():
        rep, v = gpu.g1_check(gt.to_record(x, y))
        assert v.tolist() == [gt.KIND_VERDICT[kind]], (kind, hex(x))
        assert rep["first_bad"] == (0 if gt.KIND_VERDICT[kind] else UINT64_MAX)
    good, _ = _split()
    recs = [good[i % len(good)] for i in range(130)]
    rep, v = gpu.g1_check(_bytes(recs))
    assert not v.any() and rep == _expect(recs)[0] and rep["n_infinity"] > 0


def test_three_forms_give_equal_verdicts(gpu):
    """valid, infinity, off-curve and torsion records in Montgomery form and in the MSM's converted form (noncanonical records have no
    such form: the conversions reduce); Montgomery records with p added are noncanonical there too"""
    pool = [(x, y) for k, x, y in gt.check_inputs() if k != "noncanonical"]
    recs = [pool[i % len(pool)] for i in range(100)]
    want_rep, want_v = _expect(recs)
    plain = _bytes(recs)
    rep, v = gpu.g1_check(plain)
    assert rep == want_rep and (v == want_v).all()
    mont = [gt.to_montgomery(x, y) for x, y in recs]
    rep_m, v_m = gpu.g1_check(_bytes(mont), bases_form=gpu.BASES_MONTGOMERY)
    assert rep_m == want_rep and (v_m == want_v).all()
    conv = gpu.msm_convert_bases(plain, len(recs))
    rep_c, v_c = gpu.g1_check(conv, bases_form=gpu.BASES_CONVERTED)
    assert rep_c == want_rep and (v_c == want_v).all()
    # x R + p is not x R: noncanonical in the Montgomery form as well, whatever the point was
    mx, my = gt.to_montgomery(*gt.G)
    shifted = [(mx + gt.P, my), (mx, my + gt.P), (mx, my)]
    rep_s, v_s = gpu.g1_check(_bytes(shifted), bases_form=gpu.BASES_MONTGOMERY)
    assert v_s.tolist() == [gt.BAD_NONCANONICAL, gt.BAD_NONCANONICAL, 0] and rep_s["n_noncanonical"] == 2 and rep_s["first_bad"] == 0
    conv_host = np.asarray(conv.to_host()).copy()
    cx, cy = gt.from_record(conv_host[:96])                              # record 0 of the pool is a valid point
    assert want_v[0] == 0
    conv_host[:96] = gt.to_record(cx + gt.P, cy)
    rep_k, v_k = gpu.g1_check(conv_host, bases_form=gpu.BASES_CONVERTED)
    assert v_k[0] == gt.BAD_NONCANONICAL and (v_k[1:] == want_v[1:]).all()


def test_strided_view(gpu):
    good, bad = _split()
    valid = [g for g in good if g != (0, 0)]
    rows, cols, stride = 3, 5, 8
    table = [valid[i % len(valid)] for i in range(rows * stride)]
    table[1 * stride + 6] = bad[0]                                       # outside the view: columns 5..7 are not read
    table[2 * stride + 7] = bad[3]
    rep, v = gpu.g1_check(_bytes(table), cols=cols, stride=stride)
    assert rep == _expect([valid[0]] * (rows * cols))[0] and not v.any() and v.size == rows * cols
    torsion = next((x, y) for k, x, y in gt.check_inputs() if k == "torsion" and x)
    table[1 * stride + 2] = torsion                                      # inside: view index 1 * cols + 2
    table[2 * stride + 4] = bad[0]
    rep, v = gpu.g1_check(_bytes(table), cols=cols, stride=stride)
    view = [table[a * stride + b] for a in range(rows) for b in range(cols)]
    want_rep, want_v = _expect(view)
    assert want_rep["first_bad"] == 1 * cols + 2 and want_v[2 * cols + 4] == gt.verdict(*bad[0]) != 0
    assert rep == want_rep and (v == want_v).all()
    # the contiguous call over the same table sees the records the view left out
    rep_all, v_all = gpu.g1_check(_bytes(table))
    assert (v_all == _expect(table)[1]).all() and v_all[1 * stride + 6] != 0 and v_all[2 * stride + 7] != 0


def test_refusals(gpu):
    rec = gt.to_record(*gt.G)
    with pytest.raises(gpu.TkmkError) as e:
        gpu.g1_check(rec, bases_form=gpu.BASES_ACC_READY)
    assert e.value.code == 11
    for cols, stride in ((5, 0), (0, 8), (8, 5)):
        with pytest.raises(gpu.TkmkError) as e:
            gpu.g1_check(np.tile(rec, 16), cols=cols, stride=stride, n=1)
        assert e.value.code == 11
    rep = gpu.G1CheckReport()
    assert gpu.lib().tkmk_g1_check(None, 0, ctypes.c_uint64(4), 0, 0, None, ctypes.byref(rep), None) == 3      # TKMK_ERR_INVALID_POINTER
    assert gpu.lib().tkmk_g1_check(None, 0, ctypes.c_uint64(0), 0, 0, None, None, None) == 3


def test_entry_changes_no_library_state(gpu, oracle):
    n = 96
    s, p = oracle.fr_random(901, n), oracle.g1_random_bases(902, n)
    before = np.asarray(gpu.msm(s, p)).copy()
    gen = gpu.root_generator()
    _, bad = _split()
    gpu.g1_check(_bytes(_layout(65, bad)))
    gpu.profile_enable(True)
    gpu.profile_reset()
    gpu.g1_check(_bytes(_layout(65, bad)), want_verdicts=False)
    ms, count = gpu.profile_get("g1.check")
    gpu.profile_enable(False)
    assert count == 1 and ms > 0
    assert (np.asarray(gpu.msm(s, p)) == before).all() and gpu.root_generator() == gen
    assert (gpu.projective_to_affine_bytes(before) == oracle.g1_msm(s, p)).all()
