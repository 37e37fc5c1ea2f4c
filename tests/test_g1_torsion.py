"""not-gpu tier: the generators of tests/g1_torsion.py deliver what they claim, its verdict function agrees with the oracle on curve
membership, and the shortcut csrc/g1check.hip takes — Scott's endomorphism test with a DERIVED beta — decides exactly [r]P = infinity on
every input of tests/test_gpu_g1_check.py."""
import random

import numpy as np

import g1_torsion as gt


def test_torsion_builders_deliver_their_orders():
    rng = random.Random(7)
    for ell in gt.COFACTOR_PRIMES:
        assert gt.H % ell == 0
        t = gt.torsion_point(ell, rng)
        assert t is not None and gt.on_curve(t)
        assert gt.mul(ell, t) is None                     # order divides the prime ell and is not 1: exactly ell
        assert gt.mul(gt.R, t) is not None                # not in the prime-order subgroup
        s = gt.add(gt.G, t)
        assert gt.on_curve(s) and gt.mul(gt.R, s) is not None and gt.mul(gt.R * ell, s) is None
    assert gt.on_curve((0, 2)) and gt.mul(3, (0, 2)) is None
    q = gt.random_curve_point(rng)
    assert gt.on_curve(q)
    assert gt.mul(gt.R, gt.G) is None and gt.mul(gt.H * gt.R, q) is None


def test_claimed_kinds_are_the_reference_verdicts():
    kinds = set()
    for kind, x, y in gt.check_inputs():
        assert gt.verdict(x, y) == gt.KIND_VERDICT[kind], (kind, hex(x), hex(y))
        kinds.add(kind)
    assert kinds == set(gt.KIND_VERDICT)


def test_verdict_agrees_with_the_oracle_on_curve_membership(oracle):
    for kind, x, y in gt.check_inputs():
        if kind in ("infinity", "noncanonical"):          # the oracle's predicate takes canonical finite points
            continue
        assert oracle.g1_on_curve(gt.to_record(x, y)) == (gt.verdict(x, y) != gt.BAD_OFF_CURVE), (kind, hex(x))
    base = oracle.g1_random_bases(4101, 2)
    assert gt.verdict(*gt.from_record(base[:96])) == 0 and oracle.g1_on_curve(base[:96])


def test_beta_is_derived_and_the_endomorphism_rule_is_the_subgroup_rule():
    beta = gt.derive_beta()
    assert beta == 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFE
    assert (beta * beta + beta + 1) % gt.P == 0
    other = beta * beta % gt.P
    n_in = 0
    for kind, x, y in gt.check_inputs():
        if kind in ("infinity", "noncanonical", "off_curve"):   # the rule is applied to finite curve points only
            continue
        member = gt.in_subgroup((x, y))
        n_in += member
        assert gt.endomorphism_accepts((x, y)) == member, (kind, hex(x))
        assert not gt.endomorphism_accepts((x, y), beta=other)  # the other root accepts nothing
    assert n_in >= 9


def test_montgomery_records_round_trip():
    x, y = gt.G
    mx, my = gt.to_montgomery(x, y)
    inv = pow(1 << 384, -1, gt.P)
    assert (mx * inv % gt.P, my * inv % gt.P) == gt.G
    assert gt.from_record(gt.to_record(mx, my)) == (mx, my)
    assert isinstance(gt.to_record(0, 0), np.ndarray) and not gt.to_record(0, 0).any()
