// hostcheck_signed_add.cpp — TEST-ONLY: ecu::add_mixed_signed and the accumulate-ready table row (csrc/ec_u.h) on the host, with every
// FFU_ASSERT bound check live.  Built on its own by build_signed_add.py (the unit is fully unrolled curve code: slow to compile).
#include "hostcheck_common.h"
#include "ec_u.h"

using P = bls12_381_fq_params;
using F = ff<P>;
using FU = ffu<P>;
using GU = ecu<P>;
using G = ec<F>;
static const size_t SZ = 4 * F::N;

static typename F::E ksat() {
    typename F::E k;
    for (int i = 0; i < F::N; i++) k.l[i] = P::KSAT[i];
    return k;
}
// plain 96-byte affine record -> the converted record k_convert_bases / k_precompute_bases write ((0, 0) stays infinity)
static affine_t<F> converted(const uint8_t *pt) {
    affine_t<F> rec;
    load<F>(rec.x, pt);
    load<F>(rec.y, pt + SZ);
    if (!(F::is_zero(rec.x) && F::is_zero(rec.y))) rec.x = F::mul(rec.x, ksat()), rec.y = F::mul(rec.y, ksat());
    return rec;
}
static bool same_sat(const xyzz_t<F> &a, const xyzz_t<F> &b) {
    if (G::is_inf(a) || G::is_inf(b)) return G::is_inf(a) && G::is_inf(b);
    return F::eq(a.x, b.x) && F::eq(a.y, b.y) && F::eq(a.zz, b.zz) && F::eq(a.zzz, b.zzz);
}
static void store_affine_plain(uint8_t *out, const xyzz_t<F> &r) {
    affine_t<F> a = G::to_affine(r);
    store<F>(out, F::from_mont(a.x));
    store<F>(out + SZ, F::from_mont(a.y));
}

extern "C" {
// pair i: accumulator = pts[i] + pts[i + 1] (ZZ, ZZZ != 1), base = pts[i + 2], sign = signs[i].  Returns the number of pairs on which
// to_sat(add_mixed_signed(acc, q, s)) differs from to_sat(add_mixed(acc, s ? neg(q) : q)); out (96 bytes per pair) = the affine sum.
// first = 1: the accumulator is infinity (the first entry of a bucket).
size_t hc_signed_add_pairs(const uint8_t *pts, const uint8_t *signs, size_t pairs, int first, uint8_t *out) {
    size_t bad = 0;
    for (size_t i = 0; i < pairs; i++) {
        typename GU::A a0, a1, q;
        GU::load_affine(a0, converted(pts + 2 * SZ * i));
        GU::load_affine(a1, converted(pts + 2 * SZ * (i + 1)));
        GU::load_affine(q, converted(pts + 2 * SZ * (i + 2)));
        typename GU::X acc = first ? GU::inf() : GU::add_mixed(GU::add_mixed(GU::inf(), a0), a1);
        const bool s = signs[i] != 0;
        xyzz_t<F> got = GU::to_sat(GU::add_mixed_signed(acc, q, s));
        xyzz_t<F> want = GU::to_sat(GU::add_mixed(acc, s ? GU::neg(q) : q));
        if (!same_sat(got, want)) bad++;
        store_affine_plain(out + 2 * SZ * i, got);
    }
    return bad;
}
// accumulator given as four strict 14-limb values (any residues: the formulas are polynomial identities, so the two adders must agree
// off the curve too) — the extremes of the invariant, X just below 5.03 p and Y, ZZ, ZZZ just below 1.03 p.  1 = agree.
int hc_signed_add_limbs(const uint32_t *acc_limbs, const uint8_t *pt, int sign) {
    typename GU::X acc;
    acc.inf = false;
    for (int i = 0; i < FU::L; i++) {
        acc.x.l[i] = acc_limbs[i], acc.y.l[i] = acc_limbs[FU::L + i];
        acc.zz.l[i] = acc_limbs[2 * FU::L + i], acc.zzz.l[i] = acc_limbs[3 * FU::L + i];
    }
    typename GU::A q;
    GU::load_affine(q, converted(pt));
    xyzz_t<F> got = GU::to_sat(GU::add_mixed_signed(acc, q, sign != 0));
    xyzz_t<F> want = GU::to_sat(GU::add_mixed(acc, sign ? GU::neg(q) : q));
    return same_sat(got, want) ? 1 : 0;
}
// P == +-Q: accumulator = a + b built by the mixed adder, base = `sum` (the affine a + b); through the slow path.  out = affine result of
// the signed adder; returns 1 when it equals ec.h's own mixed addition of the signed base on the saturated form.
int hc_signed_add_same_x(const uint8_t *a, const uint8_t *b, const uint8_t *sum, int sign, uint8_t *out) {
    typename GU::A qa, qb, q;
    GU::load_affine(qa, converted(a));
    GU::load_affine(qb, converted(b));
    GU::load_affine(q, converted(sum));
    typename GU::X acc = GU::add_mixed(GU::add_mixed(GU::inf(), qa), qb);
    xyzz_t<F> got = GU::to_sat(GU::add_mixed_signed(acc, q, sign != 0));
    affine_t<F> qs;
    qs.x = FU::to_sat_mont(q.x);
    qs.y = FU::to_sat_mont(q.y);
    if (sign) qs.y = F::neg(qs.y);
    xyzz_t<F> want = G::add_mixed(GU::to_sat(acc), qs);
    affine_t<F> ga = G::to_affine(got), wa = G::to_affine(want);
    store_affine_plain(out, got);
    return (G::is_inf(got) == G::is_inf(want)) && F::eq(ga.x, wa.x) && F::eq(ga.y, wa.y);
}
// accumulate-ready row: to_row of the converted record, read back by load_row, against load_affine of the record itself.  Returns the
// number of records that differ (presence, any limb, a non-zero padding word, or a row that is not one 128-byte line).
size_t hc_row_roundtrip(const uint8_t *pts, size_t n) {
    size_t bad = 0;
    if (sizeof(typename GU::Row) != 128 || alignof(typename GU::Row) != 128) return n + 1;
    for (size_t i = 0; i < n; i++) {
        affine_t<F> rec = converted(pts + 2 * SZ * i);
        typename GU::A q1, q2;
        const bool h1 = GU::load_affine(q1, rec);
        typename GU::Row row = GU::to_row(rec);
        const bool h2 = GU::load_row(q2, row);
        bool ok = h1 == h2;
        if (h1 && h2)
            for (int l = 0; l < FU::L; l++) ok = ok && q1.x.l[l] == q2.x.l[l] && q1.y.l[l] == q2.y.l[l];
        for (int w = 2 * F::N; w < 32; w++) ok = ok && row.w[w] == 0;
        if (!ok) bad++;
    }
    return bad;
}
}
