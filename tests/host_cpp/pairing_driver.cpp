// test driver for host/tkmk_pairing.hpp, stand-alone (no device entry is called).  No arguments: self-check of the tower on fixed inputs —
// Fp6 / Fp12 ring identities, inverse, complex squaring against the product, the sparse line product against the full one, Frobenius
// against a^p, Frobenius^12 = id, multiplicativity; the final exponentiation of a non-unit has order dividing r and is not 1; the pairing
// of the standard generators is not 1, has order r and is bilinear; G1 / G2 subgroup checks — one "ok <name>" line each, exit status 1 at
// the first failure.  "product": reads lines "<g1 record hex, 96 bytes> <g2 record hex, 192 bytes>" from stdin and prints 1 / 0 for "the product of
// the pairings is 1" after the checks a verifier owes its inputs, or "refused <index> <reason>".
#include <cstdio>
#include <iostream>
#include <sstream>

#include "tkmk_pairing.hpp"

using namespace tkmk;
using namespace tkmk::pairing;

static Fq fq_of(const char *hex) {   // big-endian hex, no prefix
    std::string h = hex;
    u64 l[N] = {};
    for (size_t k = 0; k < h.size(); k++) {
        char c = h[h.size() - 1 - k];
        u64 v = c >= '0' && c <= '9' ? c - '0' : c - 'a' + 10;
        l[k / 16] |= v << (4 * (k % 16));
    }
    return g2h::from_plain(l);
}
static F2 f2_fixed(u64 seed) { return {g2h::mul(g2h::small(seed * 7919 + 13), g2h::small(seed + 104729)), g2h::inv(g2h::small(seed * 31 + 5))}; }
static F6 f6_fixed(u64 s) { return {f2_fixed(s), f2_fixed(s + 100), f2_fixed(s + 200)}; }
static F12 f12_fixed(u64 s) { return {f6_fixed(s), f6_fixed(s + 1000)}; }
static F12 f12_add(const F12 &a, const F12 &b) { return {f6_add(a.c0, b.c0), f6_add(a.c1, b.c1)}; }

static int failures = 0;
static void expect(bool ok, const char *name) {
    printf("%s %s\n", ok ? "ok" : "FAILED", name);
    if (!ok) failures++;
}

static std::vector<uint8_t> bytes_of(const std::string &h) {
    if (h.size() % 2) throw Error("odd hex length");
    std::vector<uint8_t> b(h.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    return b;
}

static int product_mode() {
    std::vector<Pair> pairs;
    std::string line;
    size_t idx = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string ph, qh;
        if (!(is >> ph >> qh)) continue;
        auto pb = bytes_of(ph), qb = bytes_of(qh);
        if (pb.size() != 96 || qb.size() != 192) throw Error("a line is a 96-byte and a 192-byte record");
        tkmk_g1_affine rec;
        std::memcpy(&rec, pb.data(), 96);
        Pair pr;
        const char *why = g1_check(rec, pr.p);
        if (!*why) why = g2_check(qb.data(), pr.q);
        if (*why) {
            printf("refused %zu %s\n", idx, why);
            return 0;
        }
        pairs.push_back(pr);
        idx++;
    }
    printf("%d\n", product_is_one(pairs) ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc > 1 && std::string(argv[1]) == "product") return product_mode();
        const F12 a = f12_fixed(1), b = f12_fixed(2), c = f12_fixed(3), one = f12_one();
        const F6 x6 = f6_fixed(7), y6 = f6_fixed(8), z6 = f6_fixed(9);
        expect(f6_mul(f6_mul(x6, y6), z6) == f6_mul(x6, f6_mul(y6, z6)), "fp6 associativity");
        expect(f6_mul(x6, f6_add(y6, z6)) == f6_add(f6_mul(x6, y6), f6_mul(x6, z6)), "fp6 distributivity");
        expect(f6_mul(x6, f6_inv(x6)) == f6_one(), "fp6 inverse");
        expect(f6_mul_v(x6) == f6_mul(x6, F6{f2_zero(), f2_one(), f2_zero()}), "fp6 times v");
        expect(f6_mul_01(x6, y6.a0, y6.a1) == f6_mul(x6, F6{y6.a0, y6.a1, f2_zero()}), "fp6 sparse product");
        {
            F6 v{f2_zero(), f2_one(), f2_zero()};
            expect(f6_mul(f6_mul(v, v), v) == F6{F2{g2h::one(), g2h::one()}, f2_zero(), f2_zero()}, "v^3 = 1 + u");
            F12 w{f6_zero(), f6_one()};
            expect(f12_mul(w, w) == F12{v, f6_zero()}, "w^2 = v");
        }
        expect(f12_mul(f12_mul(a, b), c) == f12_mul(a, f12_mul(b, c)), "fp12 associativity");
        expect(f12_mul(a, b) == f12_mul(b, a), "fp12 commutativity");
        expect(f12_mul(a, f12_add(b, c)) == f12_add(f12_mul(a, b), f12_mul(a, c)), "fp12 distributivity");
        expect(f12_sqr(a) == f12_mul(a, a), "fp12 squaring");
        expect(f12_mul(a, f12_inv(a)) == one && !(a == one), "fp12 inverse");
        {
            F2 l0 = f2_fixed(41), l2 = f2_fixed(42);
            Fq l3 = g2h::small(4242);
            F12 line{{l0, l2, f2_zero()}, {f2_zero(), F2{l3, g2h::zero()}, f2_zero()}};
            expect(f12_mul_line(a, l0, l2, l3) == f12_mul(a, line), "fp12 sparse line product");
        }
        expect(f12_frob(a) == f12_pow(a, g2h::MODQ, N), "frobenius = a^p");
        expect(f12_frob(f12_mul(a, b)) == f12_mul(f12_frob(a), f12_frob(b)), "frobenius multiplicative");
        {
            F12 t = a;
            for (int i = 0; i < 6; i++) t = f12_frob(t);
            expect(t == f12_conj(a), "frobenius^6 = conjugation");
            for (int i = 0; i < 6; i++) t = f12_frob(t);
            expect(t == a, "frobenius^12 = id");
        }
        {
            F12 e = final_exponentiation(a);
            expect(!(e == one), "final exponentiation of a non-unit is not 1");
            expect(f12_pow(e, frh::MOD.l, 4) == one, "final exponentiation has order dividing r");
            expect(final_exponentiation(f12_mul(a, b)) == f12_mul(e, final_exponentiation(b)), "final exponentiation multiplicative");
        }
        // the standard generators of G1 and G2
        G1Aff g{};
        g.x = fq_of("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb");
        g.y = fq_of("08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1");
        g2h::Affine h{};
        h.x = {fq_of("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8"),
               fq_of("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e")};
        h.y = {fq_of("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801"),
               fq_of("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be")};
        expect(g1_on_curve(g) && g1_in_subgroup(g), "G1 generator on the curve, in the subgroup");
        expect(g2h::on_curve(h) && g2_in_subgroup(h), "G2 generator on the twist, in the subgroup");
        {
            G1Aff r = g1_to_affine(g1_mul(fr_from_u32(6), g)), s = g1_to_affine(g1_add(g1_dbl(g1_dbl(g1_to_jac(g))), g1_dbl(g1_to_jac(g))));
            expect(r.x == s.x && r.y == s.y && g1_on_curve(r), "G1 scalar multiplication");
            G1Aff back;
            expect(g1_decode(g1_encode(r), back) && back.x == r.x && back.y == r.y, "G1 record round trip");
            G1Aff off{};   // (0, 2) is on the curve (4 = 0 + 4) but E(Fp) has a cofactor
            off.x = g2h::zero(), off.y = g2h::small(2);
            expect(g1_on_curve(off) && !g1_in_subgroup(off), "G1 subgroup check refuses a point of the cofactor");
        }
        F12 e = final_exponentiation(miller_loop({{g, h}}));
        expect(!(e == one), "e(G, H) is not 1");
        expect(f12_pow(e, frh::MOD.l, 4) == one, "e(G, H) has order r");
        G1Aff g2x = g1_to_affine(g1_mul(fr_from_u32(2), g)), g6n = g1_neg(g1_to_affine(g1_mul(fr_from_u32(6), g)));
        g2h::Affine h3 = g2h::scalar_mul(fr_from_u32(3), h);
        expect(final_exponentiation(miller_loop({{g2x, h3}})) == f12_mul(f12_mul(f12_sqr(e), f12_sqr(e)), f12_sqr(e)), "e(2G, 3H) = e(G, H)^6");
        expect(product_is_one({{g2x, h3}, {g6n, h}}), "e(2G, 3H) e(-6G, H) = 1");
        expect(!product_is_one({{g2x, h3}, {g1_neg(g1_to_affine(g1_mul(fr_from_u32(5), g))), h}}), "e(2G, 3H) e(-5G, H) is not 1");
        G1Aff inf{};
        inf.inf = true;
        g2h::Affine inf2{};
        inf2.inf = true;
        expect(product_is_one({}) && product_is_one({{inf, h}, {g, inf2}}), "empty product and pairs with infinity are 1");
        return failures ? 1 : 0;
    } catch (const std::exception &ex) {
        fprintf(stderr, "pairing_driver: %s\n", ex.what());
        return 2;
    }
}
