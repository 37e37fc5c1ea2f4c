"""Big-integer helper for the membership tests of tkmk_g1_check (tests/test_g1_torsion.py, tests/test_gpu_g1_check.py): affine arithmetic
on E(Fp): y^2 = x^3 + 4 of BLS12-381, builders of points OUTSIDE the prime-order subgroup (one of every prime order that divides the
cofactor), a sampler of random curve points, and the reference verdict: canonical, then curve, then [r]P = infinity — the rule of
g1_in_subgroup in host/tkmk_pairing.hpp, with no shortcut.  Points are (x, y) tuples of Python integers, None = infinity."""
import functools
import random

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
Z = -0xD201000000010000                      # the curve parameter
assert R == Z**4 - Z**2 + 1 and P == (Z - 1) ** 2 * R // 3 + Z
H = (Z - 1) ** 2 // 3                        # cofactor: #E(Fp) = H * R
COFACTOR_PRIMES = (3, 11, 10177, 859267, 52437899)
G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
BAD_NONCANONICAL, BAD_OFF_CURVE, BAD_NOT_IN_SUBGROUP = 1, 2, 4


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 4) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def mul(k, pt):
    if k < 0:
        return mul(-k, neg(pt))
    acc = None
    while k and pt is not None:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def random_curve_point(rng):
    """a uniform point of E(Fp) (p = 3 mod 4: y = rhs^((p + 1) / 4) where rhs is a square); almost never in the subgroup"""
    while True:
        x = rng.randrange(P)
        rhs = (x**3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return (x, y if rng.random() < 0.5 else -y % P)


def torsion_point(ell, rng):
    """a point of exact order ell, ell a prime dividing the cofactor: [#E / ell^k]Q has order a power of ell; walk it down to ell"""
    n, k = H * R, 0
    while n % ell == 0:
        n //= ell
        k += 1
    assert k >= 1
    while True:
        t = mul(n, random_curve_point(rng))
        if t is None:
            continue
        while mul(ell, t) is not None:
            t = mul(ell, t)
        return t


def in_subgroup(pt):
    return mul(R, pt) is None


@functools.lru_cache(maxsize=None)
def verdict(x, y):
    """the reference verdict of one PLAIN record given by its stored integers: 0 for infinity (0, 0) and for members of the subgroup, else
    the first failing test"""
    if x == 0 and y == 0:
        return 0
    if x >= P or y >= P:
        return BAD_NONCANONICAL
    if not on_curve((x, y)):
        return BAD_OFF_CURVE
    return 0 if in_subgroup((x, y)) else BAD_NOT_IN_SUBGROUP


@functools.lru_cache(maxsize=None)
def derive_beta():
    """the cube root of unity beta in Fp with (beta x, y) = [-z^2 mod r](x, y) on the subgroup, found from the generator (not typed in)"""
    c = 2
    while pow(c, (P - 1) // 3, P) == 1:
        c += 1
    w = pow(c, (P - 1) // 3, P)
    assert w != 1 and pow(w, 3, P) == 1
    target = mul(-Z * Z % R, G)
    fits = [b for b in (w, w * w % P) if (b * G[0] % P, G[1]) == target]
    assert len(fits) == 1
    return fits[0]


def endomorphism_accepts(pt, beta=None):
    """Scott's test (ePrint 2021/1130) as csrc/g1check.hip computes it: two [|z|] chains, then (beta x, y) == -[z^2]P"""
    if pt is None:
        return True
    beta = derive_beta() if beta is None else beta
    q = mul(-Z, mul(-Z, pt))
    return q is not None and (beta * pt[0] % P, pt[1]) == neg(q)


def to_record(x, y):
    """96-byte record of the stored integers (little-endian, 48 bytes each); x, y < 2^384"""
    return np.frombuffer(int(x).to_bytes(48, "little") + int(y).to_bytes(48, "little"), np.uint8).copy()


def from_record(rec):
    b = bytes(rec)
    return int.from_bytes(b[:48], "little"), int.from_bytes(b[48:96], "little")


def to_montgomery(x, y):
    """the stored integers of the Montgomery form (R = 2^384) of a canonical record; infinity stays (0, 0)"""
    return x * (1 << 384) % P, y * (1 << 384) % P


@functools.lru_cache(maxsize=None)
def check_inputs():
    """the input mix of the GPU test, as (kind, x, y) with kind in {"valid", "infinity", "off_curve", "noncanonical", "torsion"}: what the
    helper CLAIMS each record is; tests/test_g1_torsion.py asserts the claims against verdict() without a GPU"""
    import oracle
    rng = random.Random(20211130)
    base = oracle.g1_random_bases(4101, 6)
    valid = [from_record(base[96 * i:96 * i + 96]) for i in range(6)]
    valid += [G, mul(2, G), mul(R - 1, G)]
    valid += [neg(v) for v in valid[:3]] + [neg(G)]
    out = [("valid", x, y) for x, y in valid]
    out.append(("infinity", 0, 0))
    for x, y in valid[:2]:
        out.append(("off_curve", x, (y + 1) % P))
        out.append(("off_curve", y, x))
        out.append(("noncanonical", x + P, y))
        out.append(("noncanonical", x, y + P))
    out += [("torsion", 0, 2), ("torsion", 0, P - 2)]
    for ell in COFACTOR_PRIMES:
        t = torsion_point(ell, rng)
        out.append(("torsion", *t))
        out.append(("torsion", *add(G, t)))
    out.append(("torsion", *random_curve_point(rng)))   # order divisible by a cofactor prime except with probability ~ 1 / H
    return tuple(out)


KIND_VERDICT = {"valid": 0, "infinity": 0, "off_curve": BAD_OFF_CURVE, "noncanonical": BAD_NONCANONICAL, "torsion": BAD_NOT_IN_SUBGROUP}
