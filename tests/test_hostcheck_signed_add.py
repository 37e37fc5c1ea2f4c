"""not-gpu tier: ecu::add_mixed_signed (the sign of a sorted entry folded into the one subtraction y enters) and the accumulate-ready
128-byte table row of csrc/ec_u.h, compiled for the HOST with every FFU_ASSERT bound check live (tests/hostcheck/hostcheck_signed_add.cpp):
a violated bound of the comment table in ec_u.h aborts the process."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
L, W = 14, 29          # strict limbs of the BLS12-381 base field (csrc/field_params.h: LU, WU)


@pytest.fixture(scope="module")
def hs():
    spec = importlib.util.spec_from_file_location("hostcheck_build_signed_add", os.path.join(HERE, "hostcheck", "build_signed_add.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = mod.build()
    assert so is not None, "hipcc is needed to compile the host check"
    lib = ctypes.CDLL(so)
    lib.hc_signed_add_pairs.restype = ctypes.c_size_t
    lib.hc_row_roundtrip.restype = ctypes.c_size_t
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _limbs(v):
    """integer -> strict form: 13 limbs of 29 bits, the top limb holds the rest"""
    out = [(v >> (W * i)) & ((1 << W) - 1) for i in range(L - 1)]
    out.append(v >> (W * (L - 1)))
    assert out[-1] < (1 << 29)
    return out


def test_signed_add_equals_add_of_negated_base_on_random_pairs(hs, oracle):
    """>= 10^4 random (accumulator, base, sign) triples: add_mixed_signed(acc, q, s) == add_mixed(acc, s ? neg(q) : q) after to_sat,
    and a sample of the sums against the oracle's group law"""
    pairs = 10240
    pts = oracle.g1_random_bases(0x5161, pairs + 2)
    rnd = random.Random(11)
    signs = np.array([rnd.randrange(2) for _ in range(pairs)], np.uint8)
    out = np.empty(96 * pairs, np.uint8)
    bad = hs.hc_signed_add_pairs(_p(pts), _p(signs), ctypes.c_size_t(pairs), 0, _p(out))
    assert bad == 0
    P = lambda i: pts[96 * i:96 * (i + 1)].copy()
    for i in list(range(40)) + [pairs - 1]:
        q = P(i + 2)
        want = oracle.g1_add(oracle.g1_add(P(i), P(i + 1)), oracle.g1_neg(q) if signs[i] else q)
        assert (out[96 * i:96 * (i + 1)] == want).all(), i
    # the first entry of a bucket: the accumulator is infinity, the sum is the signed base itself
    bad = hs.hc_signed_add_pairs(_p(pts), _p(signs), ctypes.c_size_t(256), 1, _p(out))
    assert bad == 0
    for i in range(256):
        q = P(i + 2)
        assert (out[96 * i:96 * (i + 1)] == (oracle.g1_neg(q) if signs[i] else q)).all(), i


def test_signed_add_at_the_extremes_of_the_accumulator_invariant(hs, oracle):
    """X just below 5.03 p; Y, ZZ, ZZZ just below 1.03 p (and the other end, small values): both signs agree with the unsigned adder and
    no bound assertion of ffu.h / ec_u.h fires.  The accumulator need not be on the curve: the two adders are the same polynomials."""
    p = oracle.P_MOD
    rnd = random.Random(12)
    pts = oracle.g1_random_bases(0x5162, 8)
    hi_x, hi_1 = 503 * p // 100, 103 * p // 100
    cases = []
    for k in range(64):
        d = [rnd.randrange(1, 1 << rnd.choice((1, 16, 64, 200, 370))) for _ in range(4)]
        cases.append((hi_x - d[0], hi_1 - d[1], hi_1 - d[2], hi_1 - d[3]))          # all at the top
        cases.append((hi_x - d[0], d[1], hi_1 - d[2], d[3]))                            # mixed
        cases.append((d[0], hi_1 - d[1], d[2], hi_1 - d[3]))
        cases.append((d[0] + 1, d[1] + 1, d[2] + 1, d[3] + 1))                          # all at the bottom
        cases.append((4 * p + d[0] % p, p + d[1] % (3 * p // 100), p - 1 - d[2] % p, p + d[3] % (3 * p // 100)))   # around multiples of p
    for n, (x, y, zz, zzz) in enumerate(cases):
        acc = np.array(_limbs(x) + _limbs(y) + _limbs(zz) + _limbs(zzz), np.uint32)
        q = pts[96 * (n % 8):96 * (n % 8 + 1)].copy()
        for s in (0, 1):
            assert hs.hc_signed_add_limbs(_p(acc), _p(q), s) == 1, (n, s)


def test_signed_add_same_x_goes_through_the_slow_path(hs, oracle):
    """P == Q (doubling) and P == -Q (cancellation), reached with either sign: decided on the saturated form, equal to ec.h and the oracle"""
    pts = oracle.g1_random_bases(0x5163, 12)
    out = np.empty(96, np.uint8)
    for i in range(0, 12, 2):
        a, b = pts[96 * i:96 * (i + 1)].copy(), pts[96 * (i + 1):96 * (i + 2)].copy()
        s = oracle.g1_add(a, b)
        twice = oracle.g1_add(s, s)
        for base, sign, want in ((s, 0, twice), (s, 1, np.zeros(96, np.uint8)), (oracle.g1_neg(s), 1, twice), (oracle.g1_neg(s), 0, np.zeros(96, np.uint8))):
            assert hs.hc_signed_add_same_x(_p(a), _p(b), _p(base), sign, _p(out)) == 1
            assert (out == want).all()


def test_accumulate_ready_row_reads_back_as_the_packed_record(hs, oracle):
    """row -> G1U::A equals load_affine of the 96-byte converted record, (0, 0) infinity records included; padding words are zero"""
    n = 4096
    pts = oracle.g1_random_bases(0x5164, n).copy()
    for i in (0, 17, n - 1):
        pts[96 * i:96 * (i + 1)] = 0
    assert hs.hc_row_roundtrip(_p(pts), ctypes.c_size_t(n)) == 0
