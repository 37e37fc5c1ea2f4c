"""Big-integer definition of the unsaturated Montgomery products of csrc/ffu.h (mul, mul_add, mul_add<true>, sqr) and the operand set the
host check (tests/test_ffu_reference.py) and the device check (tests/test_gpu_ffu_device.py) share.

The result is defined exactly, not only modulo p:  t = a b [+ c d],  R = 2^(W L),  m = t (-p^-1) mod R,  r = (t + m p) / R  (the division
is exact), written as strict limbs: L - 1 limbs of W bits, the top limb holds the rest.  Operands are raw limb vectors; their value is
sum l[i] 2^(W i) whether or not the limbs are strict (the c of mul_add<true> is not)."""
import functools
import math
import random

import numpy as np

MUL, MUL_ADD, MUL_ADD_UNSWEPT, SQR = 0, 1, 2, 3
OPS = (MUL, MUL_ADD, MUL_ADD_UNSWEPT, SQR)
OP_NAMES = {MUL: "mul", MUL_ADD: "mul_add", MUL_ADD_UNSWEPT: "mul_add_unswept", SQR: "sqr"}
NEEDS = {MUL: 2, MUL_ADD: 4, MUL_ADD_UNSWEPT: 4, SQR: 1}
# curve (the index tkmk_diag_ffu takes) -> modulus, limbs, bits per limb (csrc/field_params.h: LU, WU)
FIELDS = {
    0: dict(name="bls12_381_fq", L=14, W=29,
            p=0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB),
    1: dict(name="bn254_fq", L=10, W=28, p=21888242871839275222246405745257275088696311157297823662689037894645226208583),
}
RANDOM_TUPLES = 1024


def limbs(v, L, W):
    """integer -> strict limbs (the top limb holds the rest)"""
    out = [(v >> (W * i)) & ((1 << W) - 1) for i in range(L - 1)] + [v >> (W * (L - 1))]
    assert out[-1] < (1 << 32)
    return out


def value(l, W):
    return sum(int(x) << (W * i) for i, x in enumerate(l))


def sub2(p, L, W):
    """2p in the dominating-limb form of ffu::sub<2> / neg2_unswept (tools/gen_field_params.py:sub_const)"""
    d = limbs(2 * p, L, W)
    c = [d[0] + (1 << W)] + [d[i] + (1 << W) - 1 for i in range(1, L - 1)] + [d[L - 1] - 1]
    assert value(c, W) == 2 * p
    return c


def reference(curve, op, a, b=None, c=None, d=None):
    """exact result limbs of one tuple of raw limb vectors"""
    f = FIELDS[curve]
    p, L, W = f["p"], f["L"], f["W"]
    R = 1 << (W * L)
    t = value(a, W) ** 2 if op == SQR else value(a, W) * value(b, W)
    if op in (MUL_ADD, MUL_ADD_UNSWEPT):
        t += value(c, W) * value(d, W)
    m = t * (-pow(p, -1, R)) % R
    q, rem = divmod(t + m * p, R)
    assert rem == 0
    return limbs(q, L, W)


def edge_values(curve):
    f = FIELDS[curve]
    p, L, W = f["p"], f["L"], f["W"]
    low = (1 << (W * (L - 1))) - 1                        # the lower L - 1 limbs all MASK
    fullest = ((((1 << 10) * p - 1 - low) >> (W * (L - 1))) << (W * (L - 1))) + low   # largest such value below 2^10 p
    assert fullest < (1 << 10) * p and limbs(fullest, L, W)[:-1] == [(1 << W) - 1] * (L - 1)
    return [0, 1, (1 << (W * L)) % p, p - 1, p, p + 1, 2 * p - 1, 503 * p // 100 - 1, 903 * p // 100 - 1, fullest]


def unswept_values(curve):
    """raw limb vectors a neg2_unswept() can hand mul_add<true> as c: every lower limb 2^(W+1) - 1 under the top limb of the dominating
    form of 2p (25 for BLS12-381 Fq), and 2p - y limb by limb for the edge values y below 1.03 p (the Y1 of ec_u.h)"""
    f = FIELDS[curve]
    p, L, W = f["p"], f["L"], f["W"]
    s2 = sub2(p, L, W)
    out = [[(1 << (W + 1)) - 1] * (L - 1) + [s2[-1]]]
    for y in edge_values(curve):
        if 100 * y < 103 * p:
            out.append([s2[i] - yl for i, yl in enumerate(limbs(y, L, W))])
    for l in out:
        assert all(0 <= x < (1 << (W + 1)) for x in l)
    return out


@functools.lru_cache(maxsize=None)
def operand_set(curve, op):
    """(a, b, c, d) as (n, L) uint32 arrays (None where the op reads no such operand) and the (n, L) reference limbs.  Edge tuples: the
    cross product of the edge values for (a, b); for the two mul_add forms every (a, b) pair against a permutation of the (c, d) pairs and
    900 seeded draws from the four-way cross product; then RANDOM_TUPLES seeded random tuples.  Every tuple keeps a b + c d < 2^20 p^2."""
    f = FIELDS[curve]
    p, L, W = f["p"], f["L"], f["W"]
    rnd = random.Random(0xFF0 + 16 * curve + op)
    E = [limbs(v, L, W) for v in edge_values(curve)]
    C = unswept_values(curve) if op == MUL_ADD_UNSWEPT else E
    need = NEEDS[op]

    def rand_strict():
        k = rnd.choice((1, 1, 2, 6, 10, 1 << 10))        # below p, 2p, 6p, 10p, 2^10 p
        return limbs(rnd.randrange(k * p), L, W)

    def rand_c():
        if op != MUL_ADD_UNSWEPT:
            return rand_strict()
        return [rnd.randrange(1 << (W + 1)) for _ in range(L - 1)] + [rnd.randrange(sub2(p, L, W)[-1] + 1)]

    tuples = []
    if need == 1:
        tuples += [(a,) for a in E]
    elif need == 2:
        tuples += [(a, b) for a in E for b in E]
    else:
        ab = [(a, b) for a in E for b in E]
        cd = [(c, d) for c in C for d in E]
        assert math.gcd(37, len(cd)) == 1 and len(cd) <= len(ab)
        tuples += [ab[t] + cd[(37 * t + 11) % len(cd)] for t in range(len(ab))]
        tuples += [(rnd.choice(E), rnd.choice(E), rnd.choice(C), rnd.choice(E)) for _ in range(900)]
    for _ in range(RANDOM_TUPLES):
        tuples.append(tuple([rand_strict(), rand_strict(), rand_c(), rand_strict()][:need]))
    bound = (1 << 20) * p * p

    def total(t):
        v = [value(x, W) for x in t]
        return v[0] * v[0] if need == 1 else v[0] * v[1] + (v[2] * v[3] if need == 4 else 0)

    tuples = [t for t in tuples if total(t) < bound]
    ops = [np.array([t[k] for t in tuples], np.uint32) if k < need else None for k in range(4)]
    want = np.array([reference(curve, op, *t) for t in tuples], np.uint32)
    for x in ops + [want]:
        if x is not None:
            x.setflags(write=False)
    return ops, want
