// ec_u.h — XYZZ mixed addition (madd-2008-s, 8M + 2S) on the unsaturated field representation (ffu.h); the
// hot loop of the MSM bucket accumulation.  Same group law and the same degenerate-case behaviour as ec.h
// (P == Q doubles, P == -Q and infinity handled); the rare degenerate cases leave the fast path and run through
// the saturated implementation (ec.h), so there is a single place where they are decided.
//
// Value bounds (multiples of p; every operand of a product must stay below 2^10 p, every subtrahend below the K of
// its sub<K>).  Products return < 1.03 p.  With the accumulator invariant X1 < 5.03p, Y1, ZZ1, ZZZ1 < 1.03p:
//   U2 = X2 ZZ1, S2 = Y2 ZZZ1                    < 1.03
//   P  = U2 - X1  (sub<8>)   in (2.97, 9.03)     == 0 mod p  <=>  P in {3p..9p}
//   R  = S2 - Y1  (sub<2>)   in (0.97, 3.03)
//   PP = P^2, PPP = P PP, Q = X1 PP              < 1.03
//   X3 = R^2 - (PPP + 2Q)  (sub<4>, t < 3.09)    < 5.03      (invariant restored)
//   Y3 = [R (Q - X3) + (2p - Y1) PPP] / R'       < 1.03      (sub<8>, sub<2>; ONE reduction for both products)
//   ZZ3 = ZZ1 PP, ZZZ3 = ZZZ1 PPP                < 1.03
// add_mixed_signed (the base enters as +Q or -Q, decided by a mask, no negated copy of y is made): only R changes,
//   R  = +-S2 - Y1  (sub2_signed)   + : S2 + (2p - Y1)        in (0.97, 3.03)
//                                   - : (2p - S2) + (2p - Y1) in (1.94, 4.00]      so R in (0.97, 4.03) whatever the sign
//   R enters R^2 and R (Q - X3) only, as an operand of a product: 4.03 p is far below the 2^10 p operand bound and its top limb
//   (<= 4.03 * 13) far below 2^29; both products return < 1.03 p, so X3 = R^2 - t (sub<4>, t < 3.09) < 5.03 and Y3 < 1.03 as before:
//   the accumulator invariant and the K of every sub<K> downstream are those of add_mixed.
//   (2p - Y1) is used once, as the operand c of mul_add against the strict PPP: it is taken WITHOUT its carry sweep (neg2_unswept: limbs
//   SUB2[i] - Y1[i] < 2^30, top limb <= 25).  A column of mul_add then holds L products < 2^58 (a b), L < 2^59 (c d) and L < 2^58
//   (m p): 14 * 2^59 + 2 * 14 * 2^58 = 56 * 2^58 < 2^64, checked by FFU_ASSERT on the host; the value is still 2p - Y1 < 2p.
#pragma once
#include <type_traits>

#include "ec.h"
#include "ffu.h"

template <class P>
struct ecu {
    using FU = ffu<P>;
    using FS = ff<P>;
    using GS = ec<FS>;
    using E = typename FU::E;
    struct A {  // affine base: strict, canonical (< p), Montgomery radix 2^(W L); never infinity on the fast path
        E x, y;
    };
    struct X {
        E x, y, zz, zzz;
        bool inf;
    };

    static FF_HD X inf() {
        X r;
        r.x = FU::zero();
        r.y = FU::zero();
        r.zz = FU::zero();
        r.zzz = FU::zero();
        r.inf = true;
        return r;
    }
    // packed record written by k_convert_bases: {x 2^(W L) mod p, y 2^(W L) mod p} as 32-bit limbs; (0,0) = infinity
    static FF_HD bool load_affine(A &q, const affine_t<FS> &rec) {
        if (FS::is_zero(rec.x) && FS::is_zero(rec.y)) return false;
        q.x = FU::from_packed(rec.x);
        q.y = FU::from_packed(rec.y);
        return true;
    }
    static FF_HD A neg(const A &q) {
        A r;
        r.x = q.x;
        E m;
#pragma unroll
        for (int i = 0; i < FU::L; i++) m.l[i] = P::MODU[i];
        // p - y, limb-wise with one borrow sweep (y canonical, y != 0 on the curve y^2 = x^3 + b with b != 0 ... y = 0
        // cannot occur in the prime-order subgroup; p - 0 = p would still be a valid redundant value)
        E t;
        uint32_t br = 0;
#pragma unroll
        for (int i = 0; i < FU::L; i++) {
            uint32_t d = m.l[i] - q.y.l[i] - br;
            br = d >> 31;
            t.l[i] = i < FU::L - 1 ? (d & FU::MASK) : d;
        }
        r.y = t;
        return r;
    }
    // q or -q by mask (m = 0 or all ones): the borrow sweep of neg() with its result merged by and / or, no select and no branch
    static FF_HD A neg_masked(const A &q, uint32_t m) {
        A n = neg(q), r;
        r.x = q.x;
#pragma unroll
        for (int i = 0; i < FU::L; i++) r.y.l[i] = (q.y.l[i] & ~m) | (n.y.l[i] & m);
        return r;
    }

    // ---- accumulate-ready table rows (TKMK_BASES_ACC_READY): one 128-byte record on a 128-byte boundary per table row, so that a
    // gathered row is ONE cache line instead of a 96-byte record that straddles two.  The packed {x R', y R'} words of the converted
    // record (words [0, N) and [N, 2N)), the rest zero.  Infinity is marked in band: word N - 1 (the top word of x, below 2^30 for any
    // canonical x of the fields served here) is all ones — one compare in the loop instead of the OR over 2N words.
    // (Measured against rows of pre-unpacked strict limbs, which lose: tools/experiments/r05_acc_row_unpacked_limbs.patch.)
    struct alignas(128) Row {
        uint32_t w[32];
    };
    static_assert(2 * FS::N <= 32, "row does not fit its line");
    static constexpr uint32_t ROW_INF = 0xffffffffu;
    static FF_HD Row to_row(const affine_t<FS> &rec) {
        Row r;
#pragma unroll
        for (int i = 0; i < 32; i++) r.w[i] = 0;
#pragma unroll
        for (int i = 0; i < FS::N; i++) r.w[i] = rec.x.l[i], r.w[FS::N + i] = rec.y.l[i];
        if (FS::is_zero(rec.x) && FS::is_zero(rec.y)) r.w[FS::N - 1] = ROW_INF;
        return r;
    }
    // what a table kernel stores for the converted record `a`, by the type of its output
    static FF_HD void to_record(affine_t<FS> &r, const affine_t<FS> &a) { r = a; }
    static FF_HD void to_record(Row &r, const affine_t<FS> &a) { r = to_row(a); }
    static FF_HD bool load_row(A &q, const Row &r) {
        typename FS::E x, y;
#pragma unroll
        for (int i = 0; i < FS::N; i++) x.l[i] = r.w[i], y.l[i] = r.w[FS::N + i];
        q.x = FU::from_packed(x);
        q.y = FU::from_packed(y);
        return r.w[FS::N - 1] != ROW_INF;
    }
    static FF_HD X from_affine(const A &q) {
        X r;
        r.x = q.x;
        r.y = q.y;
        r.zz = FU::one();
        r.zzz = FU::one();
        r.inf = false;
        return r;
    }

    // unsaturated XYZZ -> saturated Montgomery XYZZ (what the combine / reduce kernels and the host consume)
    static FF_HD xyzz_t<FS> to_sat(const X &p) {
        xyzz_t<FS> r;
        if (p.inf) return GS::inf();
        r.x = FU::to_sat_mont(p.x);
        r.y = FU::to_sat_mont(p.y);
        r.zz = FU::to_sat_mont(p.zz);
        r.zzz = FU::to_sat_mont(p.zzz);
        return r;
    }
    // "raw" record: the unsaturated coordinates as they are (x R' mod p, redundant: X < 5.03p, the others < 1.03p — both
    // fit the 32N-bit words), normalised and packed, all-zero = infinity.  Writing it costs no multiplication, which
    // matters inside the accumulate loop: lanes leave a bucket at different iterations, so a flush is executed by the
    // whole wave for one or two active lanes; the four conversion products of to_sat() are done later, convergently,
    // by whoever reads the record (raw_to_sat).
    static FF_HD xyzz_t<FS> to_raw(const X &p) {
        xyzz_t<FS> r;
        if (p.inf) return GS::inf();
        r.x = FU::pack(FU::norm(p.x));
        r.y = FU::pack(FU::norm(p.y));
        r.zz = FU::pack(FU::norm(p.zz));
        r.zzz = FU::pack(FU::norm(p.zzz));
        return r;
    }
    static FF_HD xyzz_t<FS> raw_to_sat(const xyzz_t<FS> &raw) {
        if (FS::is_zero(raw.zz)) return GS::inf();   // zz == 0 exactly only for the infinity record (zz != 0 mod p otherwise)
        xyzz_t<FS> r;
        r.x = FU::to_sat_mont(FU::unpack(raw.x));
        r.y = FU::to_sat_mont(FU::unpack(raw.y));
        r.zz = FU::to_sat_mont(FU::unpack(raw.zz));
        r.zzz = FU::to_sat_mont(FU::unpack(raw.zzz));
        return r;
    }
    // raw record -> unsaturated point: unpack only (the bounds of to_raw's inputs carry over)
    static FF_HD X from_raw(const xyzz_t<FS> &raw) {
        X r;
        r.inf = FS::is_zero(raw.zz);
        if (r.inf) return inf();
        r.x = FU::unpack(raw.x);
        r.y = FU::unpack(raw.y);
        r.zz = FU::unpack(raw.zz);
        r.zzz = FU::unpack(raw.zzz);
        return r;
    }
    static FF_HD E from_sat_mont(const typename FS::E &s) {  // x 2^(32N) canonical -> x 2^(W L) strict canonical
        typename FS::E k;
#pragma unroll
        for (int i = 0; i < FS::N; i++) k.l[i] = P::KSATM[i];
        return FU::unpack(FS::mul(s, k));
    }
    static FF_HD X from_sat(const xyzz_t<FS> &p) {
        X r;
        r.inf = GS::is_inf(p);
        if (r.inf) return inf();
        r.x = from_sat_mont(p.x);
        r.y = from_sat_mont(p.y);
        r.zz = from_sat_mont(p.zz);
        r.zzz = from_sat_mont(p.zzz);
        return r;
    }
    // degenerate cases: decide and compute on the saturated representation (ec.h handles P == Q, P == -Q)
    static FF_HD X add_mixed_slow(const X &p, const A &q) {
        affine_t<FS> qs;
        qs.x = FU::to_sat_mont(q.x);
        qs.y = FU::to_sat_mont(q.y);
        return from_sat(GS::add_mixed(to_sat(p), qs));
    }

    // general addition (add-2008-s, 12M + 2S, one shared reduction) for the combine / bucket-reduction kernels.  With both
    // operands in the accumulator invariant (X < 5.03p, Y, ZZ, ZZZ < 1.03p):
    //   U1 = X1 ZZ2, U2 = X2 ZZ1, S1 = Y1 ZZZ2, S2 = Y2 ZZZ1      < 1.03
    //   P = U2 - U1 (sub<2>), R = S2 - S1 (sub<2>)                 in (0.97, 3.03);  P == 0 mod p <=> P in {p, 2p, 3p}
    //   X3 = R^2 - (PPP + 2Q)  (sub<4>)  < 5.03;  Y3 = [R (Q - X3) + (2p - S1) PPP]/R' < 1.03;  ZZ3, ZZZ3 < 1.03
    static FF_HD X add_slow(const X &p, const X &q) { return from_sat(GS::add(to_sat(p), to_sat(q))); }
    static FF_HD X add(const X &p, const X &q) {
        if (p.inf) return q;
        if (q.inf) return p;
        E u1 = FU::mul(p.x, q.zz), u2 = FU::mul(q.x, p.zz);
        E s1 = FU::mul(p.y, q.zzz), s2 = FU::mul(q.y, p.zzz);
        E pd = FU::template sub<2>(u2, u1);
        if (FU::maybe_multiple_of_p(pd, 3)) return add_slow(p, q);   // same x: doubling or cancellation, decided in ec.h
        E rd = FU::template sub<2>(s2, s1);
        E pp = FU::sqr(pd);
        E ppp = FU::mul(pd, pp);
        E qq = FU::mul(u1, pp);
        X r;
        r.inf = false;
        r.x = FU::template sub<4>(FU::sqr(rd), FU::add_dbl(ppp, qq));
        r.y = FU::mul_add(rd, FU::template sub<8>(qq, r.x), FU::template sub<2>(FU::zero(), s1), ppp);
        r.zz = FU::mul(FU::mul(p.zz, q.zz), pp);
        r.zzz = FU::mul(FU::mul(p.zzz, q.zzz), ppp);
        return r;
    }
    // doubling (dbl-2008-s-1, a = 0): U = 2Y1 < 2.06, V = U^2, W = U V, S = X1 V, M = 3 X1^2 < 3.09,
    //   X3 = M^2 - 2S (sub<4>) < 5.03,  Y3 = [M (S - X3) + (2p - W) Y1]/R' < 1.03,  ZZ3 = V ZZ1, ZZZ3 = W ZZZ1
    static FF_HD X dbl(const X &p) {
        if (p.inf) return p;
        E u = FU::dbl(p.y);
        E v = FU::sqr(u);
        E w = FU::mul(u, v);
        E sx = FU::mul(p.x, v);
        E x2 = FU::sqr(p.x);
        E m = FU::add(FU::dbl(x2), x2);
        X r;
        r.inf = false;
        r.x = FU::template sub<4>(FU::sqr(m), FU::dbl(sx));
        r.y = FU::mul_add(m, FU::template sub<8>(sx, r.x), FU::template sub<2>(FU::zero(), w), p.y);
        r.zz = FU::mul(v, p.zz);
        r.zzz = FU::mul(w, p.zzz);
        return r;
    }

    // p + q, q an affine point (not infinity)
    static FF_HD X add_mixed(const X &p, const A &q) {
        if (p.inf) return from_affine(q);
        E u2 = FU::mul(q.x, p.zz);
        E s2 = FU::mul(q.y, p.zzz);
        E pd = FU::template sub<8>(u2, p.x);
        // P == 0 mod p  <=>  P = j p with 3 <= j <= 9: only then can q share its x with the accumulator
        if (FU::maybe_multiple_of_p(pd, 9)) return add_mixed_slow(p, q);
        E rd = FU::template sub<2>(s2, p.y);
        E pp = FU::sqr(pd);
        E ppp = FU::mul(pd, pp);
        E qq = FU::mul(p.x, pp);
        X r;
        r.inf = false;
        E t = FU::add_dbl(ppp, qq);
        r.x = FU::template sub<4>(FU::sqr(rd), t);
        E d = FU::template sub<8>(qq, r.x);
        r.y = FU::mul_add(rd, d, FU::template sub<2>(FU::zero(), p.y), ppp);  // R (Q - X3) + (2p - Y1) PPP, one reduction
        r.zz = FU::mul(p.zz, pp);
        r.zzz = FU::mul(p.zzz, ppp);
        return r;
    }
    // p + q or p - q (negate), q an affine point (not infinity): add_mixed with the sign folded into the one subtraction that y enters
    // (see the bounds at the top); the rare cases that need a negated copy of q make it there
    static FF_HD X add_mixed_signed(const X &p, const A &q, bool negate) { return add_mixed_masked(p, q, 0u - (uint32_t)negate); }
    // the same with the sign as a mask (0 or all ones).  The accumulate kernel makes it from the sorted record by an arithmetic shift: a
    // mask made from a bool is folded back into selects by the compiler (14 v_cndmask_b32 in sub2_signed, seen in the ISA).
    static FF_HD X add_mixed_masked(const X &p, const A &q, uint32_t m) {
        if (p.inf) return from_affine(neg_masked(q, m));
        E u2 = FU::mul(q.x, p.zz);
        E s2 = FU::mul(q.y, p.zzz);
        E pd = FU::template sub<8>(u2, p.x);
        if (FU::maybe_multiple_of_p(pd, 9)) return add_mixed_slow(p, neg_masked(q, m));
        E rd = FU::sub2_signed(s2, p.y, m);
        E pp = FU::sqr(pd);
        E ppp = FU::mul(pd, pp);
        E qq = FU::mul(p.x, pp);
        X r;
        r.inf = false;
        E t = FU::add_dbl(ppp, qq);
        r.x = FU::template sub<4>(FU::sqr(rd), t);
        E d = FU::template sub<8>(qq, r.x);
        r.y = FU::template mul_add<true>(rd, d, FU::neg2_unswept(p.y), ppp);
        r.zz = FU::mul(p.zz, pp);
        r.zzz = FU::mul(p.zzz, ppp);
        return r;
    }
};

using G1U = ecu<bls12_381_fq_params>;
