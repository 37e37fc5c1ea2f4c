// tkmk_pairing.hpp — the BLS12-381 pairing on the host, for the verifier (host/tkmk_verify.hpp): the counterpart of `pairing` of the
// reference's libs/src/group_structures, which verify-rust/src/lib.rs:248-352 calls ten times per proof.  Host-only on purpose: one
// verification is ~25 G1 scalar multiplications, one ten-pair Miller loop and one final exponentiation — about 0.1 s on one core with
// the plain Montgomery arithmetic of tkmk_g2.hpp, most of it membership checks — and a verifier also runs where there is no GPU.
// Header-only, over the Montgomery Fq / Fp2 of tkmk_g2.hpp.
//
//   tower     Fp2 = Fp[u]/(u^2 + 1) (tkmk_g2.hpp), Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v), xi = 1 + u; so w^6 = xi, and an Fp12
//             element is sum_k a_k w^k with a_k in Fp2: a_0, a_2, a_4 = c0.a0, c0.a1, c0.a2 and a_1, a_3, a_5 = c1.a0, c1.a1, c1.a2
//   twist     M-type, E'(Fp2): y^2 = x^3 + 4 xi; (x', y') -> (x' / w^2, y' / w^3) lands on E(Fp12): y^2 = x^3 + 4
//   Miller    optimal ate, loop count |x| = 0xd201000000010000, affine steps on the twist with ONE Fp2 inversion per step for all pairs
//             (Montgomery's trick); the line through T with twist slope m, evaluated at P = (xP, yP) and scaled by w^3 (an element of
//             Fp4, which the final exponentiation kills): (m xT - yT) - (m xP) w^2 + yP w^3 — three of the six Fp2 coefficients, so a
//             sparse product; the squarings of f are shared by all pairs; x < 0: the result is conjugated
//   final     easy part (p^6 - 1)(p^2 + 1), then the hard part through 3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3
//             (Hayashida, Hayasaka, Teruya, "Efficient final exponentiation via cyclotomic structure for pairings over families of elliptic
//             curves", 2020): the map is the CUBE of the reduced ate pairing — still bilinear and non-degenerate since 3 does not divide r
// Only the decision "the product of the pairings is 1" is exposed; nothing depends on the representation of GT.
// Frobenius constants xi^(k (p - 1) / 6) are computed at start-up from the modulus, like every other constant of the host arithmetic.
// Inputs of miller_loop / product_is_one must be on their curves and in the r-torsion (g1_check / g2_check): the affine steps assume
// that no intermediate multiple of Q is +-Q or of order two, which holds for points of prime order r.
#pragma once
#include <utility>

#include "tkmk_g2.hpp"

namespace tkmk {
namespace pairing {

using g2h::F2;
using g2h::Fq;
using g2h::u64;
constexpr int N = g2h::N;

// ---- Fp, Fp2 helpers on top of tkmk_g2.hpp ----
inline Fq fq_neg(const Fq &a) { return g2h::sub(g2h::zero(), a); }
inline Fq fq_dbl(const Fq &a) { return g2h::add(a, a); }
inline F2 f2_zero() { return {g2h::zero(), g2h::zero()}; }
inline F2 f2_one() { return {g2h::one(), g2h::zero()}; }
inline F2 f2_neg(const F2 &a) { return {fq_neg(a.c0), fq_neg(a.c1)}; }
inline F2 f2_conj(const F2 &a) { return {a.c0, fq_neg(a.c1)}; }
inline F2 f2_dbl(const F2 &a) { return {fq_dbl(a.c0), fq_dbl(a.c1)}; }
inline F2 f2_sq(const F2 &a) {   // (a0 + a1)(a0 - a1) + 2 a0 a1 u
    Fq t = g2h::mul(a.c0, a.c1);
    return {g2h::mul(g2h::add(a.c0, a.c1), g2h::sub(a.c0, a.c1)), fq_dbl(t)};
}
inline F2 f2_mul_fq(const F2 &a, const Fq &k) { return {g2h::mul(a.c0, k), g2h::mul(a.c1, k)}; }
inline F2 f2_mul_xi(const F2 &a) { return {g2h::sub(a.c0, a.c1), g2h::add(a.c0, a.c1)}; }   // (a0 + a1 u)(1 + u)
using g2h::f2_add;
using g2h::f2_inv;
using g2h::f2_is_zero;
using g2h::f2_mul;
using g2h::f2_sub;
// a^e, e little-endian 64-bit limbs
inline F2 f2_pow(const F2 &a, const u64 *e, int limbs) {
    F2 r = f2_one();
    for (int i = 64 * limbs - 1; i >= 0; i--) {
        r = f2_sq(r);
        if ((e[i / 64] >> (i % 64)) & 1) r = f2_mul(r, a);
    }
    return r;
}

// ---- Fp6 = Fp2[v] / (v^3 - xi) ----
struct F6 {
    F2 a0, a1, a2;
    bool operator==(const F6 &o) const { return a0 == o.a0 && a1 == o.a1 && a2 == o.a2; }
};
inline F6 f6_zero() { return {f2_zero(), f2_zero(), f2_zero()}; }
inline F6 f6_one() { return {f2_one(), f2_zero(), f2_zero()}; }
inline F6 f6_add(const F6 &a, const F6 &b) { return {f2_add(a.a0, b.a0), f2_add(a.a1, b.a1), f2_add(a.a2, b.a2)}; }
inline F6 f6_sub(const F6 &a, const F6 &b) { return {f2_sub(a.a0, b.a0), f2_sub(a.a1, b.a1), f2_sub(a.a2, b.a2)}; }
inline F6 f6_neg(const F6 &a) { return {f2_neg(a.a0), f2_neg(a.a1), f2_neg(a.a2)}; }
inline F6 f6_mul_v(const F6 &a) { return {f2_mul_xi(a.a2), a.a0, a.a1}; }
inline F6 f6_mul(const F6 &a, const F6 &b) {   // Karatsuba, 6 Fp2 products
    F2 t0 = f2_mul(a.a0, b.a0), t1 = f2_mul(a.a1, b.a1), t2 = f2_mul(a.a2, b.a2);
    F2 c0 = f2_add(t0, f2_mul_xi(f2_sub(f2_sub(f2_mul(f2_add(a.a1, a.a2), f2_add(b.a1, b.a2)), t1), t2)));
    F2 c1 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a1), f2_add(b.a0, b.a1)), t0), t1), f2_mul_xi(t2));
    F2 c2 = f2_add(f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a2), f2_add(b.a0, b.a2)), t0), t2), t1);
    return {c0, c1, c2};
}
// a * (b0 + b1 v): 5 Fp2 products
inline F6 f6_mul_01(const F6 &a, const F2 &b0, const F2 &b1) {
    F2 t0 = f2_mul(a.a0, b0), t1 = f2_mul(a.a1, b1);
    F2 c0 = f2_add(t0, f2_mul_xi(f2_mul(a.a2, b1)));
    F2 c1 = f2_sub(f2_sub(f2_mul(f2_add(a.a0, a.a1), f2_add(b0, b1)), t0), t1);
    F2 c2 = f2_add(f2_mul(a.a2, b0), t1);
    return {c0, c1, c2};
}
inline F6 f6_inv(const F6 &a) {
    F2 c0 = f2_sub(f2_sq(a.a0), f2_mul_xi(f2_mul(a.a1, a.a2)));
    F2 c1 = f2_sub(f2_mul_xi(f2_sq(a.a2)), f2_mul(a.a0, a.a1));
    F2 c2 = f2_sub(f2_sq(a.a1), f2_mul(a.a0, a.a2));
    F2 t = f2_add(f2_mul(a.a0, c0), f2_mul_xi(f2_add(f2_mul(a.a2, c1), f2_mul(a.a1, c2))));
    F2 ti = f2_inv(t);
    return {f2_mul(c0, ti), f2_mul(c1, ti), f2_mul(c2, ti)};
}

// ---- Fp12 = Fp6[w] / (w^2 - v) ----
struct F12 {
    F6 c0, c1;
    bool operator==(const F12 &o) const { return c0 == o.c0 && c1 == o.c1; }
};
inline F12 f12_one() { return {f6_one(), f6_zero()}; }
inline bool f12_is_one(const F12 &a) { return a == f12_one(); }
inline F12 f12_mul(const F12 &a, const F12 &b) {
    F6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1)), t0), t1)};
}
inline F12 f12_sqr(const F12 &a) {   // complex squaring: 2 Fp6 products
    F6 t = f6_mul(a.c0, a.c1);
    F6 s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return {f6_sub(f6_sub(s, t), f6_mul_v(t)), f6_add(t, t)};
}
inline F12 f12_conj(const F12 &a) { return {a.c0, f6_neg(a.c1)}; }   // a^(p^6)
inline F12 f12_inv(const F12 &a) {
    F6 t = f6_inv(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return {f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t))};
}
// a * (l0 + l2 w^2 + l3 w^3), l3 in Fp: the line of a Miller step (13 Fp2-size products instead of 18)
inline F12 f12_mul_line(const F12 &a, const F2 &l0, const F2 &l2, const Fq &l3) {
    F6 t0 = f6_mul_01(a.c0, l0, l2);                                                                       // c0 * (l0 + l2 v)
    F6 t1 = f6_mul_v(F6{f2_mul_fq(a.c1.a0, l3), f2_mul_fq(a.c1.a1, l3), f2_mul_fq(a.c1.a2, l3)});       // c1 * (l3 v)
    F6 s = f6_mul_01(f6_add(a.c0, a.c1), l0, F2{g2h::add(l2.c0, l3), l2.c1});
    return {f6_add(t0, f6_mul_v(t1)), f6_sub(f6_sub(s, t0), t1)};
}
struct Frobenius {
    F2 g[6];   // g[k] = xi^(k (p - 1) / 6): (a w^k)^p = conj(a) g[k] w^k
    Frobenius() {
        u64 e[N];   // (p - 1) / 6
        u64 one_[N] = {1};
        g2h::sub_raw(e, g2h::MODQ, one_);
        u64 rem = 0;
        for (int i = N - 1; i >= 0; i--) {
            g2h::u128 cur = ((g2h::u128)rem << 64) | e[i];
            e[i] = (u64)(cur / 6);
            rem = (u64)(cur % 6);
        }
        F2 xi{g2h::one(), g2h::one()};
        g[0] = f2_one();
        g[1] = f2_pow(xi, e, N);
        for (int k = 2; k < 6; k++) g[k] = f2_mul(g[k - 1], g[1]);
    }
};
inline const Frobenius &frobenius_consts() {
    static const Frobenius f;
    return f;
}
inline F12 f12_frob(const F12 &a) {
    const F2 *g = frobenius_consts().g;
    return {{f2_conj(a.c0.a0), f2_mul(f2_conj(a.c0.a1), g[2]), f2_mul(f2_conj(a.c0.a2), g[4])},
            {f2_mul(f2_conj(a.c1.a0), g[1]), f2_mul(f2_conj(a.c1.a1), g[3]), f2_mul(f2_conj(a.c1.a2), g[5])}};
}
inline F12 f12_pow(const F12 &a, const u64 *e, int limbs) {
    F12 r = f12_one();
    for (int i = 64 * limbs - 1; i >= 0; i--) {
        r = f12_sqr(r);
        if ((e[i / 64] >> (i % 64)) & 1) r = f12_mul(r, a);
    }
    return r;
}
constexpr u64 ATE_LOOP = 0xd201000000010000ull;   // |x|
// a^x for the curve parameter x = -|x|, a in the cyclotomic subgroup (inverse = conjugate)
inline F12 f12_pow_x(const F12 &a) { return f12_conj(f12_pow(a, &ATE_LOOP, 1)); }
inline F12 final_exponentiation(const F12 &f) {
    F12 e = f12_mul(f12_conj(f), f12_inv(f));          // f^(p^6 - 1)
    e = f12_mul(f12_frob(f12_frob(e)), e);             // ^(p^2 + 1): now in the cyclotomic subgroup
    F12 a = f12_mul(f12_pow_x(e), f12_conj(e));        // e^(x - 1)
    a = f12_mul(f12_pow_x(a), f12_conj(a));            // e^((x - 1)^2)
    F12 b = f12_mul(f12_pow_x(a), f12_frob(a));        // ^(x + p)
    F12 c = f12_mul(f12_mul(f12_pow_x(f12_pow_x(b)), f12_frob(f12_frob(b))), f12_conj(b));   // ^(x^2 + p^2 - 1)
    return f12_mul(c, f12_mul(f12_sqr(e), e));         // * e^3
}

// ---- G1 on the host: y^2 = x^3 + 4 over Fq ----
struct G1Aff {
    Fq x, y;
    bool inf = false;
};
struct G1Jac {
    Fq X, Y, Z;   // Z = 0: infinity
};
inline G1Jac g1_jac_inf() { return {g2h::one(), g2h::one(), g2h::zero()}; }
inline G1Jac g1_to_jac(const G1Aff &p) { return p.inf ? g1_jac_inf() : G1Jac{p.x, p.y, g2h::one()}; }
inline bool g1_on_curve(const G1Aff &p) {
    if (p.inf) return true;
    return g2h::mul(p.y, p.y) == g2h::add(g2h::mul(g2h::mul(p.x, p.x), p.x), g2h::small(4));
}
inline G1Jac g1_dbl(const G1Jac &p) {   // dbl-2009-l (a = 0)
    using namespace g2h;
    if (is_zero(p.Z)) return p;
    Fq A = mul(p.X, p.X), B = mul(p.Y, p.Y), C = mul(B, B);
    Fq t = add(p.X, B);
    Fq D = fq_dbl(sub(sub(mul(t, t), A), C));
    Fq E = add(fq_dbl(A), A);
    Fq X3 = sub(mul(E, E), fq_dbl(D));
    Fq C8 = fq_dbl(fq_dbl(fq_dbl(C)));
    return {X3, sub(mul(E, sub(D, X3)), C8), fq_dbl(mul(p.Y, p.Z))};
}
inline G1Jac g1_add(const G1Jac &p, const G1Jac &q) {   // add-2007-bl
    using namespace g2h;
    if (is_zero(p.Z)) return q;
    if (is_zero(q.Z)) return p;
    Fq Z1Z1 = mul(p.Z, p.Z), Z2Z2 = mul(q.Z, q.Z);
    Fq U1 = mul(p.X, Z2Z2), U2 = mul(q.X, Z1Z1);
    Fq S1 = mul(mul(p.Y, q.Z), Z2Z2), S2 = mul(mul(q.Y, p.Z), Z1Z1);
    if (U1 == U2) return S1 == S2 ? g1_dbl(p) : g1_jac_inf();
    Fq H = sub(U2, U1), H2 = fq_dbl(H), I = mul(H2, H2), J = mul(H, I), r = fq_dbl(sub(S2, S1)), V = mul(U1, I);
    Fq X3 = sub(sub(mul(r, r), J), fq_dbl(V));
    Fq Y3 = sub(mul(r, sub(V, X3)), fq_dbl(mul(S1, J)));
    Fq ZZ = add(p.Z, q.Z);
    Fq Z3 = mul(sub(sub(mul(ZZ, ZZ), Z1Z1), Z2Z2), H);
    return {X3, Y3, Z3};
}
inline G1Aff g1_to_affine(const G1Jac &p) {
    G1Aff a;
    if (g2h::is_zero(p.Z)) {
        a.x = a.y = g2h::zero();
        a.inf = true;
        return a;
    }
    Fq zi = g2h::inv(p.Z), zi2 = g2h::mul(zi, zi);
    a.x = g2h::mul(p.X, zi2), a.y = g2h::mul(p.Y, g2h::mul(zi2, zi));
    return a;
}
inline G1Aff g1_neg(const G1Aff &p) {
    G1Aff r = p;
    if (!p.inf) r.y = fq_neg(p.y);
    return r;
}
// [k] p, k = 256 bits as four little-endian 64-bit limbs (any integer, not reduced)
inline G1Jac g1_mul_raw(const u64 *k, const G1Aff &p) {
    G1Jac acc = g1_jac_inf(), base = g1_to_jac(p);
    for (int i = 255; i >= 0; i--) {
        acc = g1_dbl(acc);
        if ((k[i / 64] >> (i % 64)) & 1) acc = g1_add(acc, base);
    }
    return acc;
}
inline G1Jac g1_mul(const ScalarField &k, const G1Aff &p) { return g1_mul_raw(frh::load(k).l, p); }
inline bool g1_in_subgroup(const G1Aff &p) { return g2h::is_zero(g1_mul_raw(frh::MOD.l, p).Z); }   // r P = infinity (E(Fp) has a cofactor)
// sum_i k_i P_i
inline G1Aff g1_lincomb(const std::vector<std::pair<ScalarField, G1Aff>> &terms) {
    G1Jac acc = g1_jac_inf();
    for (const auto &t : terms)
        if (!t.second.inf && !fr_is_zero(t.first)) acc = g1_add(acc, g1_mul(t.first, t.second));
    return g1_to_affine(acc);
}
// the 96-byte record (x, y little-endian; all zero = infinity).  false: a coordinate is >= p
inline bool g1_decode(const tkmk_g1_affine &rec, G1Aff &out) {
    u64 l[2][N];
    std::memcpy(l[0], &rec.x, 48);
    std::memcpy(l[1], &rec.y, 48);
    u64 any = 0;
    for (int c = 0; c < 2; c++)
        for (int i = 0; i < N; i++) any |= l[c][i];
    out.inf = any == 0;
    out.x = out.y = g2h::zero();
    if (out.inf) return true;
    if (g2h::geq_raw(l[0], g2h::MODQ) || g2h::geq_raw(l[1], g2h::MODQ)) return false;
    out.x = g2h::from_plain(l[0]), out.y = g2h::from_plain(l[1]);
    return true;
}
inline tkmk_g1_affine g1_encode(const G1Aff &p) {
    tkmk_g1_affine rec{};
    if (p.inf) return rec;
    u64 l[N];
    g2h::to_plain(p.x, l);
    std::memcpy(&rec.x, l, 48);
    g2h::to_plain(p.y, l);
    std::memcpy(&rec.y, l, 48);
    return rec;
}
// record -> point with the three checks a verifier owes every group element it is handed; "" = fine, else the reason
inline const char *g1_check(const tkmk_g1_affine &rec, G1Aff &out) {
    if (!g1_decode(rec, out)) return "has a coordinate that is not reduced (>= p)";
    if (!g1_on_curve(out)) return "is not on the curve";
    if (!g1_in_subgroup(out)) return "is not in the subgroup of order r";
    return "";
}
inline bool g2_in_subgroup(const g2h::Affine &q) {
    if (q.inf) return true;
    g2h::Jac acc = g2h::jac_inf(), base = g2h::to_jac(q);
    for (int i = 255; i >= 0; i--) {
        acc = g2h::dbl(acc);
        if ((frh::MOD.l[i / 64] >> (i % 64)) & 1) acc = g2h::add(acc, base);
    }
    return f2_is_zero(acc.Z);
}
inline const char *g2_check(const uint8_t *rec192, g2h::Affine &out) {
    try {
        out = g2h::decode(rec192);
    } catch (const Error &) {
        return "has a coordinate that is not reduced (>= p)";
    }
    if (!g2h::on_curve(out)) return "is not on the twist";
    if (!g2_in_subgroup(out)) return "is not in the subgroup of order r";
    return "";
}

// ---- the Miller loop of a product, and the decision ----
struct Pair {
    G1Aff p;
    g2h::Affine q;
};
inline void f2_batch_inverse(std::vector<F2> &v) {
    if (v.empty()) return;
    std::vector<F2> prefix(v.size());
    F2 acc = f2_one();
    for (size_t i = 0; i < v.size(); i++) {
        if (f2_is_zero(v[i])) throw Error("pairing: degenerate Miller step (a G2 input is not in the subgroup of order r)");
        prefix[i] = acc;
        acc = f2_mul(acc, v[i]);
    }
    F2 ia = f2_inv(acc);
    for (size_t i = v.size(); i-- > 0;) {
        F2 t = f2_mul(ia, prefix[i]);
        ia = f2_mul(ia, v[i]);
        v[i] = t;
    }
}
// prod_i f_{x, Q_i}(P_i); a pair with an infinite member contributes 1, an empty product is 1
inline F12 miller_loop(const std::vector<Pair> &pairs) {
    std::vector<const Pair *> live;
    for (const Pair &pr : pairs)
        if (!pr.p.inf && !pr.q.inf) live.push_back(&pr);
    F12 f = f12_one();
    const size_t n = live.size();
    if (n == 0) return f;
    std::vector<F2> tx(n), ty(n), den(n);
    for (size_t i = 0; i < n; i++) tx[i] = live[i]->q.x, ty[i] = live[i]->q.y;
    auto step = [&](bool doubling) {
        for (size_t i = 0; i < n; i++) den[i] = doubling ? f2_dbl(ty[i]) : f2_sub(live[i]->q.x, tx[i]);
        f2_batch_inverse(den);
        for (size_t i = 0; i < n; i++) {
            const Pair &pr = *live[i];
            F2 num = doubling ? f2_add(f2_dbl(f2_sq(tx[i])), f2_sq(tx[i])) : f2_sub(pr.q.y, ty[i]);
            F2 m = f2_mul(num, den[i]);
            F2 l0 = f2_sub(f2_mul(m, tx[i]), ty[i]);
            f = f12_mul_line(f, l0, f2_neg(f2_mul_fq(m, pr.p.x)), pr.p.y);
            const F2 &ox = doubling ? tx[i] : pr.q.x;
            F2 x3 = f2_sub(f2_sub(f2_sq(m), tx[i]), ox);
            ty[i] = f2_sub(f2_mul(m, f2_sub(tx[i], x3)), ty[i]);
            tx[i] = x3;
        }
    };
    for (int i = 62; i >= 0; i--) {
        f = f12_sqr(f);
        step(true);
        if ((ATE_LOOP >> i) & 1) step(false);
    }
    return f12_conj(f);   // x < 0
}
inline bool product_is_one(const std::vector<Pair> &pairs) { return f12_is_one(final_exponentiation(miller_loop(pairs))); }

}  // namespace pairing
}  // namespace tkmk
