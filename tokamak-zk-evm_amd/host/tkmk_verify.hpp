// tkmk_verify.hpp — the verifier: Verifier::init + verify_snark of the reference (packages/backend/verify-rust/src/lib.rs:54-117, 119-289)
// on the host alone.  Reads what the reference's `verify` reads — setupParams.json of the subcircuit library, <synthesizer>/instance.json,
// <crs>/sigma_verify.json, <preprocess>/preprocess.json, <proof>/proof.json — replays the Fiat-Shamir transcript for thetas, kappa0, chi,
// zeta, kappa1, draws kappa2 from getrandom(), evaluates a_pub(chi, zeta) in O(l_free) from the barycentric form and decides
//   e(LHS + AUX, H) e(B, a^4) e(U, a) e(V, a^2) e(W, a^3) = e(O_pub_fix + O_pub_free, gamma) e(O_mid, eta) e(O_prv, delta) e(AUX_X, x) e(AUX_Y, y)
// as ONE product of ten pairings against 1 (host/tkmk_pairing.hpp), the right-hand G1 inputs negated.  tests/prove_ref.py:528-563 is the
// same formula in Python.  No device, no NTT domain, no libtkmk_hip.so: include/tkmk.h is used for its record types only.
//
// Two kinds of "no":
//   false   a well-formed set of documents that does not verify — the pairing product is not 1, or a G1 point of proof.json /
//           preprocess.json / sigma_verify.json is off the curve, outside the subgroup of order r (E(Fp) has a cofactor, so on-curve alone
//           does not suffice) or has a coordinate >= p, or Sigma2 is all zero (every pairing would be 1 and the check vacuous).  The
//           report carries a one-line reason.
//   error   a document that cannot be read or parsed (missing file, missing entry, bad hex, wrong count): tkmk::Error naming the file.
//
// THE ROOT OF UNITY: omega_{m_I}, omega_{s_max} and omega_{l_free} come from ONE generator g (omega_{2^32} = g^((r-1)/2^32)), and
// sigma_verify.json alone cannot tell which generator the reference string was made under (the prover finds out from xy_powers, which a
// verifier does not have).  So it is an INPUT: an explicit argument, else TKMK_FR_ROOT_GENERATOR, else the declared default
// TKMK_BLS12_381_FR_ROOT_GENERATOR (include/tkmk.h).  Exactly that one is used — never a second try, never "either" — and the report names it.
#pragma once
#include <sys/random.h>

#include <array>
#include <fstream>

#include "tkmk_json.hpp"
#include "tkmk_pairing.hpp"
#include "tkmk_transcript.hpp"

namespace tkmk {
namespace verify {

using pairing::G1Aff;

// prove/src/lib.rs:460-507 (tkmk/proofio.py PROOF_POINT_ORDER): the 19 commitments of proof.json, then the points of preprocess.json
// (preprocess/src/lib.rs:93-101) and the G1 side of SigmaVerify
enum Pt { U, V, W, O_mid, O_prv, Q_AX, Q_AY, Q_CX, Q_CY, Pi_X, Pi_Y, B, R, M_Y, M_X, N_Y, N_X, O_pub_free, A_free,
          S0, S1, O_pub_fix, CRS_G, CRS_X, CRS_Y, CRS_KL, PtCount };
constexpr int kProofPoints = 19, kPrePoints = 3;
inline const char *pt_name(int i) {
    static const char *names[PtCount] = {"U", "V", "W", "O_mid", "O_prv", "Q_AX", "Q_AY", "Q_CX", "Q_CY", "Pi_X", "Pi_Y", "B", "R", "M_Y", "M_X", "N_Y",
                                         "N_X", "O_pub_free", "A_free", "s0", "s1", "O_pub_fix", "G", "sigma_1.x", "sigma_1.y", "lagrange_KL"};
    return names[i];
}
// Sigma2 in the order of the CRS payload's G2 section (tkmk/crs.py G2_POINTS)
enum G2Pt { H, Alpha, Alpha2, Alpha3, Alpha4, Gamma, Delta, Eta, X2, Y2, G2Count };
inline const char *g2_name(int i) {
    static const char *names[G2Count] = {"H", "alpha", "alpha2", "alpha3", "alpha4", "gamma", "delta", "eta", "x", "y"};
    return names[i];
}

struct Shape {   // the entries of setupParams.json a verifier uses
    size_t n = 0, l = 0, l_D = 0, s_max = 0, l_user = 0, l_free = 0;
};
struct Inputs {
    Shape sp;
    std::vector<ScalarField> a_pub;                     // a_pub_user[:l_user] ++ a_pub_block[:l_free - l_user]
    tkmk_g1_affine pt[PtCount]{};
    std::array<std::array<uint8_t, 192>, G2Count> g2{};
    ScalarField R_eval{}, R_omegaX_eval{}, R_omegaX_omegaY_eval{}, V_eval{};
    std::string crs_label = "sigma_verify.json";        // what a reason calls the source of G, x, y, lagrange_KL and Sigma2
};
struct Report {
    uint32_t generator = 0;
    bool have_challenges = false;
    ScalarField thetas[3]{}, kappa0{}, chi{}, zeta{}, kappa1{}, a_eval{};
    bool ok = false;
    std::string reason;   // for ok == false
    std::string to_json() const {
        auto esc = [](const std::string &s) {
            std::string o;
            for (char c : s) {
                if (c == '"' || c == '\\') o.push_back('\\');
                o.push_back((unsigned char)c < 0x20 ? ' ' : c);
            }
            return o;
        };
        std::string d = "{\"generator\": " + std::to_string(generator) + ", \"ok\": " + (ok ? "true" : "false") + ", \"reason\": \"" + esc(reason) + "\"";
        if (have_challenges) {
            d += ", \"thetas\": [\"" + scalar_to_hex(thetas[0]) + "\", \"" + scalar_to_hex(thetas[1]) + "\", \"" + scalar_to_hex(thetas[2]) + "\"]";
            d += ", \"kappa0\": \"" + scalar_to_hex(kappa0) + "\", \"chi\": \"" + scalar_to_hex(chi) + "\", \"zeta\": \"" + scalar_to_hex(zeta) + "\"";
            d += ", \"kappa1\": \"" + scalar_to_hex(kappa1) + "\", \"a_eval\": \"" + scalar_to_hex(a_eval) + "\"";
        }
        return d + "}";
    }
};

// ---- the generator in effect, and roots of unity on the host ----
inline uint32_t generator_in_effect(uint32_t explicit_generator = 0) {
    if (explicit_generator) return explicit_generator;
    if (const char *e = std::getenv("TKMK_FR_ROOT_GENERATOR")) {   // the rule of the device library (csrc/ntt_impl.inc)
        const int v = std::atoi(e);
        if (v >= 2 && v < 65536) return (uint32_t)v;
    }
    return TKMK_BLS12_381_FR_ROOT_GENERATOR;
}
inline ScalarField fr_pow_wide(const ScalarField &a, const frh::U256 &e) {
    ScalarField r = fr_one();
    for (int i = 255; i >= 0; i--) {
        r = fr_mul(r, r);
        if ((e.l[i / 64] >> (i % 64)) & 1) r = fr_mul(r, a);
    }
    return r;
}
// omega_size = g^((r - 1) / size), size a power of two <= 2^32; a quadratic residue as generator is refused
inline ScalarField root_of_unity(uint32_t g, uint64_t size) {
    if (size == 0 || (size & (size - 1)) || size > (1ull << 32)) throw Error("root of unity: the size must be a power of two, at most 2^32");
    if (g < 2) throw Error("root-of-unity generator must be at least 2");
    frh::U256 e = frh::sub_raw(frh::MOD, frh::U256{{1, 0, 0, 0}});   // (r - 1) >> 32
    for (int i = 0; i < 4; i++) e.l[i] = (e.l[i] >> 32) | (i + 1 < 4 ? e.l[i + 1] << 32 : 0);
    ScalarField top = fr_pow_wide(fr_from_u32(g), e), w = top, probe = top;
    for (int i = 1; i < 32; i++) probe = fr_mul(probe, probe);   // omega_2 must be -1
    if (fr_eq(probe, fr_one())) throw Error("root-of-unity generator " + std::to_string(g) + " is a quadratic residue");
    for (uint64_t s = 1ull << 32; s > size; s >>= 1) w = fr_mul(w, w);
    return w;
}
inline ScalarField random_nonzero_scalar() {   // kappa2: ScalarCfg::generate_random (verify-rust/src/lib.rs:108)
    for (;;) {
        frh::U256 v;
        if (::getrandom(v.l, sizeof v.l, 0) != (ssize_t)sizeof v.l) throw Error("getrandom failed");
        v.l[3] &= 0x7fffffffffffffffull;
        if (frh::geq(v, frh::MOD)) continue;
        ScalarField s = frh::store(v);
        if (!fr_is_zero(s)) return s;
    }
}
// p(chi) for the polynomial of degree < n with p(omega^i) = evals[i]: sum_i evals[i] (chi^n - 1) omega^i / (n (chi - omega^i)) — one
// inversion for all denominators; chi ON the domain: the value there.  (Instance::gen_a_free_X is l_free x 1, so zeta does not enter.)
inline ScalarField eval_from_rou_evals(const std::vector<ScalarField> &evals, const ScalarField &omega, const ScalarField &chi) {
    const size_t n = evals.size();
    std::vector<ScalarField> wpow(n), prefix(n);
    ScalarField w = fr_one(), acc = fr_one();
    for (size_t i = 0; i < n; i++) {
        wpow[i] = w;
        if (fr_eq(chi, w)) return evals[i];
        prefix[i] = acc;
        acc = fr_mul(acc, fr_sub(chi, w));
        w = fr_mul(w, omega);
    }
    ScalarField inv_acc = fr_inv(acc), sum{};
    for (size_t i = n; i-- > 0;) {
        ScalarField inv_i = fr_mul(inv_acc, prefix[i]);   // 1 / (chi - omega^i)
        inv_acc = fr_mul(inv_acc, fr_sub(chi, wpow[i]));
        sum = fr_add(sum, fr_mul(evals[i], fr_mul(wpow[i], inv_i)));
    }
    ScalarField scale = fr_mul(fr_sub(fr_pow(chi, n), fr_one()), fr_inv(fr_from_u32((uint32_t)n)));
    return fr_mul(sum, scale);
}

// ---- reading the documents ----
inline bool readable(const std::string &path) { return (bool)std::ifstream(path); }
template <class F>
inline auto in_file(const char *file, F &&fn) -> decltype(fn()) {
    try {
        return fn();
    } catch (const std::exception &e) {
        throw Error(std::string(file) + ": " + e.what());
    }
}
inline Shape read_shape(const std::string &lib_dir) {
    return in_file("setupParams.json", [&] {
        json::Value jp = json::read_file(lib_dir + "/setupParams.json");
        Shape s;
        s.n = jp.at("n").as_size(), s.l = jp.at("l").as_size(), s.l_D = jp.at("l_D").as_size(), s.s_max = jp.at("s_max").as_size();
        s.l_user = jp.at("l_user").as_size(), s.l_free = jp.at("l_free").as_size();
        return s;
    });
}
inline void validate_shape(const Shape &s) {   // setup_shape / validate_setup_shape (libs/src/utils/mod.rs:21-46) + what gen_a_free_X indexes
    auto pow2 = [](size_t v) { return v && !(v & (v - 1)); };
    if (s.l_D < s.l) throw Error("Invalid setup params: l_D must be >= l.");
    if (!pow2(s.n)) throw Error("n is not a power of two.");
    if (!pow2(s.s_max)) throw Error("s_max is not a power of two.");
    if (!pow2(s.l_D - s.l)) throw Error("m_I is not a power of two.");
    if (!pow2(s.l_free)) throw Error("l_free is not a power of two.");
    if (s.l_user > s.l_free) throw Error("Invalid setup params: l_user must be <= l_free.");
}
inline std::vector<ScalarField> read_instance(const std::string &synth_dir, const Shape &sp) {
    return in_file("instance.json", [&] {
        json::Value ji = json::read_file(synth_dir + "/instance.json");
        std::vector<ScalarField> a;
        const auto &user = ji.at("a_pub_user").items(), &block = ji.at("a_pub_block").items();
        if (user.size() < sp.l_user) throw Error("a_pub_user holds fewer than l_user entries");
        if (block.size() < sp.l_free - sp.l_user) throw Error("a_pub_block holds fewer than l_free - l_user entries");
        for (size_t i = 0; i < sp.l_user; i++) a.push_back(fr_from_hex(user[i].as_string()));
        for (size_t i = 0; i < sp.l_free - sp.l_user; i++) a.push_back(fr_from_hex(block[i].as_string()));
        return a;
    });
}
// one big-endian hex number -> `bytes` little-endian bytes.  Bad hex is an error; a VALUE too large for the field is not: it comes back
// as all-ones, which the range check of the group element then refuses (the decision is false)
inline void hex_number_le(const std::string &h, uint8_t *out, size_t bytes) {
    size_t off = (h.size() >= 2 && h[0] == '0' && (h[1] == 'x' || h[1] == 'X')) ? 2 : 0;
    if (h.size() == off) throw Error("empty hex number");
    std::memset(out, 0, bytes);
    bool overflow = false;
    for (size_t k = 0; k < h.size() - off; k++) {
        char c = h[h.size() - 1 - k];
        int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (v < 0) throw Error("invalid hex digit");
        if (k / 2 < bytes) out[k / 2] |= (uint8_t)(v << (4 * (k & 1)));
        else overflow |= v != 0;
    }
    if (overflow) std::memset(out, 0xff, bytes);
}
inline void read_sigma_verify(const std::string &crs_dir, Inputs &in) {
    const std::string path = crs_dir + "/sigma_verify.json";
    if (!readable(path)) throw Error("No reference string is found. Run the Setup first (expected sigma_verify.json). [" + path + "]");
    in_file("sigma_verify.json", [&] {
        json::Value sv = json::read_file(path);
        auto g1 = [&](const json::Value &p, tkmk_g1_affine &rec) {
            hex_number_le(p.at("x").as_string(), reinterpret_cast<uint8_t *>(&rec.x), 48);
            hex_number_le(p.at("y").as_string(), reinterpret_cast<uint8_t *>(&rec.y), 48);
        };
        auto g2p = [&](const json::Value &p, std::array<uint8_t, 192> &rec) {   // 96-byte Fp2 element: real part in the low half
            hex_number_le(p.at("x").as_string(), rec.data(), 96);
            hex_number_le(p.at("y").as_string(), rec.data() + 96, 96);
        };
        g1(sv.at("G"), in.pt[CRS_G]);
        g1(sv.at("sigma_1").at("x"), in.pt[CRS_X]);
        g1(sv.at("sigma_1").at("y"), in.pt[CRS_Y]);
        g1(sv.at("lagrange_KL"), in.pt[CRS_KL]);
        g2p(sv.at("H"), in.g2[H]);
        for (int k = Alpha; k < G2Count; k++) g2p(sv.at("sigma_2").at(g2_name(k)), in.g2[k]);
        return 0;
    });
    in.crs_label = "sigma_verify.json";
}
inline FormattedEntries read_entries(const std::string &path, const char *file, const char *k1, const char *k2) {
    return in_file(file, [&] {
        json::Value j = json::read_file(path);
        FormattedEntries f;
        for (const json::Value &v : j.at(k1).items()) f.part1.push_back(v.as_string());
        for (const json::Value &v : j.at(k2).items()) f.part2.push_back(v.as_string());
        return f;
    });
}
inline void read_preprocess(const std::string &dir, Inputs &in) {
    const std::string path = dir + "/preprocess.json";
    if (!readable(path)) throw Error("No Verifier preprocess is found. Run the Preprocess first. [" + path + "]");
    FormattedEntries f = read_entries(path, "preprocess.json", "preprocess_entries_part1", "preprocess_entries_part2");
    in_file("preprocess.json", [&] {
        if (f.part1.size() != 2 * kPrePoints || f.part2.size() != 2 * kPrePoints) throw Error("unexpected preprocess entry count");
        for (int i = 0; i < kPrePoints; i++) in.pt[S0 + i] = next_point(2 * i, f);
        return 0;
    });
}
inline void read_proof(const std::string &dir, Inputs &in) {
    const std::string path = dir + "/proof.json";
    if (!readable(path)) throw Error("No proof is found. Run the Prove first. [" + path + "]");
    FormattedEntries f = read_entries(path, "proof.json", "proof_entries_part1", "proof_entries_part2");
    in_file("proof.json", [&] {
        if (f.part1.size() != 2 * kProofPoints || f.part2.size() != 2 * kProofPoints + 4) throw Error("unexpected proof entry count");
        for (int i = 0; i < kProofPoints; i++) in.pt[i] = next_point(2 * i, f);
        ScalarField *ev[4] = {&in.R_eval, &in.R_omegaX_eval, &in.R_omegaX_omegaY_eval, &in.V_eval};   // prove/src/lib.rs:504-507
        for (int i = 0; i < 4; i++) {
            auto be = unhex(f.part2[2 * kProofPoints + i]);
            if (be.size() != 32) throw Error("Invalid format");
            *ev[i] = fr_from_hex(f.part2[2 * kProofPoints + i]);
        }
        return 0;
    });
}

// ---- the combined equation ----
struct LC {   // a linear combination of the named G1 points
    std::array<ScalarField, PtCount> c{};
    static LC of(int p) {
        LC r;
        r.c[p] = fr_one();
        return r;
    }
    LC operator+(const LC &o) const {
        LC r;
        for (int i = 0; i < PtCount; i++) r.c[i] = fr_add(c[i], o.c[i]);
        return r;
    }
    LC operator-(const LC &o) const {
        LC r;
        for (int i = 0; i < PtCount; i++) r.c[i] = fr_sub(c[i], o.c[i]);
        return r;
    }
    LC operator*(const ScalarField &s) const {
        LC r;
        for (int i = 0; i < PtCount; i++) r.c[i] = fr_is_zero(c[i]) ? c[i] : fr_mul(c[i], s);
        return r;
    }
    LC neg() const { return LC{} - *this; }
    G1Aff point(const G1Aff *pts) const {
        const ScalarField one = fr_one(), minus_one = fr_neg(one);
        pairing::G1Jac acc = pairing::g1_jac_inf();
        for (int i = 0; i < PtCount; i++) {
            if (fr_is_zero(c[i]) || pts[i].inf) continue;
            if (fr_eq(c[i], one)) acc = pairing::g1_add(acc, pairing::g1_to_jac(pts[i]));
            else if (fr_eq(c[i], minus_one)) acc = pairing::g1_add(acc, pairing::g1_to_jac(pairing::g1_neg(pts[i])));
            else acc = pairing::g1_add(acc, pairing::g1_mul(c[i], pts[i]));
        }
        return pairing::g1_to_affine(acc);
    }
};

// Verifier::verify_snark.  kappa2 = nullptr: fresh randomness.  Returns rep.ok; throws only for invalid setup parameters / generator.
inline bool verify_loaded(const Inputs &in, uint32_t explicit_generator, Report &rep, const ScalarField *kappa2_in = nullptr) {
    rep = Report{};
    rep.generator = generator_in_effect(explicit_generator);
    validate_shape(in.sp);
    if (in.a_pub.size() != in.sp.l_free) throw Error("instance.json: expected l_free public inputs");
    auto refuse = [&](const std::string &why) {
        rep.ok = false, rep.reason = why;
        return false;
    };
    // Sigma2 first: an all-zero G2 set would make every pairing 1
    bool any_g2 = false;
    for (const auto &r : in.g2)
        for (uint8_t b : r) any_g2 |= b != 0;
    if (!any_g2) return refuse(in.crs_label + " holds no Sigma2 (all-zero G2 points): every pairing would be 1 and the check vacuous");
    g2h::Affine q[G2Count];
    for (int k = 0; k < G2Count; k++) {
        const std::string who = in.crs_label + ": " + (k == H ? std::string("H") : std::string("sigma_2.") + g2_name(k));
        const char *why = pairing::g2_check(in.g2[k].data(), q[k]);
        if (*why) return refuse(who + " " + why);
        if (q[k].inf) return refuse(who + " is the point at infinity");
    }
    G1Aff pts[PtCount];
    for (int i = 0; i < PtCount; i++) {
        const char *why = pairing::g1_check(in.pt[i], pts[i]);
        if (*why) return refuse((i < kProofPoints ? std::string("proof.json") : i < kProofPoints + kPrePoints ? std::string("preprocess.json") : in.crs_label) + ": " + pt_name(i) + " " + why);
    }
    // Verifier::collect_challenges (verify-rust/src/lib.rs:98-117)
    TranscriptManager tm;
    tm.add_proof0(in.pt[U], in.pt[V], in.pt[W], in.pt[Q_AX], in.pt[Q_AY], in.pt[B]);
    std::vector<ScalarField> th = tm.get_thetas();
    tm.add_proof1(in.pt[R]);
    const ScalarField k0 = tm.get_kappa0();
    tm.add_proof2(in.pt[Q_CX], in.pt[Q_CY]);
    const auto cz = tm.get_chi_zeta();
    const ScalarField chi = cz.first, zeta = cz.second;
    tm.add_proof3(in.V_eval, in.R_eval, in.R_omegaX_eval, in.R_omegaX_omegaY_eval);
    const ScalarField k1 = tm.get_kappa1();
    const ScalarField k2 = kappa2_in ? *kappa2_in : random_nonzero_scalar();
    const size_t m_i = in.sp.l_D - in.sp.l, s_max = in.sp.s_max;
    const ScalarField one = fr_one();
    const ScalarField wxi = fr_inv(root_of_unity(rep.generator, m_i)), wyi = fr_inv(root_of_unity(rep.generator, s_max));
    const ScalarField a_eval = eval_from_rou_evals(in.a_pub, root_of_unity(rep.generator, in.sp.l_free), chi);
    rep.have_challenges = true;
    rep.thetas[0] = th[0], rep.thetas[1] = th[1], rep.thetas[2] = th[2];
    rep.kappa0 = k0, rep.chi = chi, rep.zeta = zeta, rep.kappa1 = k1, rep.a_eval = a_eval;

    const ScalarField t_n = fr_sub(fr_pow(chi, in.sp.n), one), t_mi = fr_sub(fr_pow(chi, m_i), one), t_s = fr_sub(fr_pow(zeta, s_max), one);
    const ScalarField chi_1 = fr_sub(chi, one);
    const ScalarField k0_e = fr_is_zero(chi_1) ? one : fr_mul(t_mi, fr_mul(fr_inv(fr_from_u32((uint32_t)m_i)), fr_inv(chi_1)));   // K_0(chi)
    const ScalarField k1_2 = fr_mul(k1, k1), k1_3 = fr_mul(k1_2, k1), k1_4 = fr_mul(k1_2, k1_2);
    const ScalarField k2_2 = fr_mul(k2, k2), k2_3 = fr_mul(k2_2, k2);
    auto p = [](int i) { return LC::of(i); };
    const LC G = p(CRS_G);
    const LC lhs_a = p(U) * in.V_eval - p(W) + (p(V) - G * in.V_eval) * k1 - p(Q_AX) * t_n - p(Q_AY) * t_s;
    const LC F = p(B) + p(S0) * th[0] + p(S1) * th[1] + G * th[2];
    const LC Gp = p(B) + p(CRS_X) * th[0] + p(CRS_Y) * th[1] + G * th[2];
    const LC term1 = p(CRS_KL) * fr_sub(in.R_eval, one) + (Gp * in.R_eval - F * in.R_omegaX_eval) * fr_mul(k0, chi_1) +
                     (Gp * in.R_eval - F * in.R_omegaX_omegaY_eval) * fr_mul(fr_mul(k0, k0), k0_e) - p(Q_CX) * t_mi - p(Q_CY) * t_s;
    const LC lhs_c = term1 * k1_2 + (p(R) - G * in.R_eval) * k1_3 + (p(R) - G * in.R_omegaX_eval) * k2 + (p(R) - G * in.R_omegaX_omegaY_eval) * k2_2;
    const ScalarField k2k14 = fr_mul(k2, k1_4);
    const LC lhs_b = p(A_free) * fr_add(one, k2k14) - G * fr_mul(k2k14, a_eval);
    const LC lhs = lhs_b + (lhs_a + lhs_c) * k2;
    const LC aux = p(Pi_X) * fr_mul(k2, chi) + p(Pi_Y) * fr_mul(k2, zeta) + p(M_X) * fr_mul(fr_mul(k2_2, wxi), chi) + p(M_Y) * fr_mul(k2_2, zeta) +
                   p(N_X) * fr_mul(fr_mul(k2_3, wxi), chi) + p(N_Y) * fr_mul(fr_mul(k2_3, wyi), zeta);
    const LC aux_x = p(Pi_X) * k2 + p(M_X) * k2_2 + p(N_X) * k2_3;
    const LC aux_y = p(Pi_Y) * k2 + p(M_Y) * k2_2 + p(N_Y) * k2_3;
    std::vector<pairing::Pair> pairs = {{(lhs + aux).point(pts), q[H]},
                                        {pts[B], q[Alpha4]},
                                        {pts[U], q[Alpha]},
                                        {pts[V], q[Alpha2]},
                                        {pts[W], q[Alpha3]},
                                        {(p(O_pub_fix) + p(O_pub_free)).neg().point(pts), q[Gamma]},
                                        {pairing::g1_neg(pts[O_mid]), q[Eta]},
                                        {pairing::g1_neg(pts[O_prv]), q[Delta]},
                                        {aux_x.neg().point(pts), q[X2]},
                                        {aux_y.neg().point(pts), q[Y2]}};
    if (!pairing::product_is_one(pairs)) return refuse("pairing product != 1");
    rep.ok = true;
    return true;
}

// Verifier::init in the reference's order of loading (verify-rust/src/lib.rs:54-96): setup parameters, instance, sigma, preprocess, proof
inline bool verify_files(const std::string &lib_dir, const std::string &crs_dir, const std::string &synth_dir, const std::string &preprocess_dir,
                         const std::string &proof_dir, uint32_t explicit_generator, Report &rep) {
    Inputs in;
    in.sp = read_shape(lib_dir);
    validate_shape(in.sp);
    in.a_pub = read_instance(synth_dir, in.sp);
    read_sigma_verify(crs_dir, in);
    read_preprocess(preprocess_dir, in);
    read_proof(proof_dir, in);
    return verify_loaded(in, explicit_generator, rep);
}

}  // namespace verify
}  // namespace tkmk
