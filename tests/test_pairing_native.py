"""CPU tier: the host pairing of host/tkmk_pairing.hpp through tkmk_pairing_product_is_one (include/tkmk_prover.h, tkmk/verify.py) — the
decision "the product of the pairings is 1" on products whose value is known from the scalars, agreement with the Python pairing of
tests/pairing_ref.py on a handful of them (8 Python pairings in all: ~1 s each), and the refusal of every kind of invalid group element.
G is the project's pinned G1 generator, H the fixed G2 generator; multiples come from the oracle and tkmk/g2.py.  The tower itself is
self-checked by tests/host_cpp/pairing_driver (no arguments), which also runs here."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = json.load(open(os.path.join(HERE, "golden", "pins.json")))
DRIVER = os.path.join(HERE, "host_cpp", "pairing_driver")


@pytest.fixture(scope="module")
def ctx(oracle, tkmk):
    from tkmk import g2, service, verify
    R = oracle.R_MOD
    g = np.asarray(oracle.to_bytes([int(PINS["fixed_tau_g1_x"], 16), int(PINS["fixed_tau_g1_y"], 16)], 48))
    h = g2.from_hex_pair(PINS["fixed_tau_g2_x"], PINS["fixed_tau_g2_y"])

    class C:
        pass
    c = C()
    c.R, c.g, c.h, c.g2, c.verify, c.service = R, g, h, g2, verify, service
    c.G = lambda k: np.asarray(oracle.g1_scalar_mul(oracle.to_bytes([k % R], 32), g))      # [k]G as a record; k = 0 mod r: all zero
    c.H = lambda k: g2.scalar_mul(k % R, h)
    c.is_one = verify.pairing_product_is_one
    rnd = random.Random(0x70616972)
    c.a, c.b = rnd.getrandbits(255) % R, rnd.getrandbits(255) % R
    return c


def test_decisions_follow_the_scalars(ctx):
    c, a, b = ctx, ctx.a, ctx.b
    assert not c.is_one([(c.g, c.h)])                                       # non-degenerate
    assert c.is_one([])                                                      # the empty product
    assert c.is_one([(c.G(a), c.H(b)), (c.G(-a * b), c.h)])
    assert not c.is_one([(c.G(a), c.H(b)), (c.G(-(a * b + 1)), c.h)])
    # additive in each argument
    assert c.is_one([(c.G(a + b), c.h), (c.G(-a), c.h), (c.G(-b), c.h)])
    assert c.is_one([(c.g, c.H(a + b)), (c.G(-1), c.H(a)), (c.G(-1), c.H(b))])
    assert not c.is_one([(c.g, c.H(a + b)), (c.G(-1), c.H(a)), (c.G(-1), c.H(b + 1))])
    # the same pair in either order of the scalars
    assert c.is_one([(c.G(a), c.h), (c.G(-1), c.H(a))])


def test_ten_pairs_and_one_scalar_off(ctx):
    """the verifier's shape: ten pairs built to multiply to 1, then one scalar off by one"""
    c = ctx
    rnd = random.Random(10)
    s = [(rnd.getrandbits(255) % c.R, rnd.getrandbits(255) % c.R) for _ in range(9)]
    total = sum(x * y for x, y in s) % c.R
    pairs = [(c.G(x), c.H(y)) for x, y in s] + [(c.G(-total), c.h)]
    assert len(pairs) == 10 and c.is_one(pairs)
    assert not c.is_one(pairs[:9] + [(c.G(-total + 1), c.h)])
    assert not c.is_one([(c.G(s[0][0] + 1), c.H(s[0][1]))] + pairs[1:])


def test_infinity_on_either_side_contributes_one(ctx):
    c = ctx
    assert c.is_one([(None, c.h), (c.g, None)])
    assert c.is_one([(c.G(0), c.h)]) and not c.G(0).any()                     # [r]G = infinity = the all-zero record
    assert c.is_one([(None, c.h), (c.G(ctx.a), c.H(ctx.b)), (c.g, None), (c.G(-ctx.a * ctx.b), c.h)])
    assert not c.is_one([(None, c.h), (c.g, c.h)])
    assert c.is_one([(c.g, np.zeros(192, np.uint8))])                          # the 192-byte record form of a G2 point


def test_agrees_with_the_python_pairing(ctx):
    """decisions only — the two maps differ (this one is the cube of the reduced optimal ate pairing, the Python one a plain ate Miller
    loop to the power (p^12 - 1) / r) but both are non-degenerate and bilinear.  8 Python pairings."""
    import pairing_ref as pr
    c, a, b = ctx, ctx.a, ctx.b
    one = pr.F12.of(1)
    lists = [[(c.g, c.h)],
             [(c.G(a), c.H(b)), (c.G(-a * b), c.h)],
             [(c.G(a), c.H(b)), (c.G(-(a * b + 1)), c.h)],
             [(None, c.h), (c.g, None)],
             [(c.G(a + b), c.h), (c.G(-a), c.h), (c.G(-b), c.h)]]
    assert sum(1 for l in lists for p, q in l if p is not None and q is not None) == 8
    for l in lists:
        want = pr.pairing_product([(None if p is None else pr.g1_from_record(p), q) for p, q in l]) == one
        assert c.is_one(l) == want, l


def _refused(c, pairs, index, what):
    with pytest.raises(c.service.ProverError) as e:
        c.is_one(pairs)
    assert e.value.code == 11, e.value                                        # TKMK_ERR_INVALID_ARGUMENT
    assert ("point %d " % index) in str(e.value) and what in str(e.value), str(e.value)


def test_invalid_group_elements_are_refused(ctx, oracle):
    c, P = ctx, oracle.P_MOD
    rec = lambda x, y: np.frombuffer(int(x).to_bytes(48, "little") + int(y).to_bytes(48, "little"), np.uint8).copy()     # noqa: E731
    gx, gy = oracle.to_ints(c.g, 48)
    good = (c.g, c.h)
    # off the curve
    _refused(c, [good, (rec(gx, (gy + 1) % P), c.h)], 1, "not on the curve")
    # on the curve, outside the subgroup of order r: E(Fp) has a cofactor
    x = next(x for x in range(1, 100) if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == 1)
    y = pow((x ** 3 + 4) % P, (P + 1) // 4, P)                                 # p = 3 mod 4
    assert y * y % P == (x ** 3 + 4) % P
    stray = rec(x, y)
    assert oracle.g1_on_curve(stray)
    r_minus_1 = np.asarray(oracle.g1_scalar_mul(oracle.to_bytes([c.R - 1], 32), stray))
    assert not (r_minus_1 == np.asarray(oracle.g1_neg(stray))).all(), "[r]P = infinity: the point is in the subgroup after all"
    _refused(c, [(stray, c.h)], 0, "subgroup")
    # a coordinate >= p
    _refused(c, [good, good, (rec(gx + P, gy), c.h)], 2, "not reduced")
    _refused(c, [(c.g, ((c.h[0][0] + P, c.h[0][1]), c.h[1]))], 0, "not reduced")
    # a G2 record off the twist
    _refused(c, [(c.g, (c.h[0], ((c.h[1][0] + 1) % P, c.h[1][1])))], 0, "not on the twist")
    # and the refusal is not sticky
    assert not c.is_one([good])


def test_tower_self_check_driver():
    """tests/host_cpp/pairing_driver.cpp: Fp6 / Fp12 ring identities, Frobenius against a^p, the final exponentiation, bilinearity on the
    standard generators — stand-alone, the program a sanitizer build runs"""
    assert os.path.exists(DRIVER), "tests/host_cpp/pairing_driver is not built (run __graft_entry__.build())"
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.split("\n")
    assert len([l for l in lines if l.startswith("ok ")]) >= 30 and not [l for l in lines if l.startswith("FAILED")]
    for name in ("frobenius = a^p", "fp12 sparse line product", "final exponentiation has order dividing r", "e(G, H) has order r"):
        assert "ok " + name in lines


def test_driver_product_mode_matches_the_library(ctx):
    c = ctx
    line = lambda p, q: bytes(p).hex() + " " + bytes(c.g2.encode(q)).hex()     # noqa: E731
    run = lambda text: subprocess.run([DRIVER, "product"], input=text, capture_output=True, text=True, timeout=60)     # noqa: E731
    r = run(line(c.G(c.a), c.H(c.b)) + "\n" + line(c.G(-c.a * c.b), c.h) + "\n")
    assert r.returncode == 0 and r.stdout.strip() == "1", (r.stdout, r.stderr)
    r = run(line(c.g, c.h) + "\n")
    assert r.returncode == 0 and r.stdout.strip() == "0", (r.stdout, r.stderr)
