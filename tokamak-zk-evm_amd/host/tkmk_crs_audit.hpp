// tkmk_crs_audit.hpp — is this reference string well formed?  The audit behind tkmk_crs_audit_files (include/tkmk_prover.h), bin/crs-check
// and the TKMK_PROVER_CHECK_CRS=1 opt-in of tkmk_prover_open, over a CrsPayload as load_combined_sigma returns it (either container).
// The reference downloads its CRS (setup/mpc-setup/src/drive_upload.rs, prove/src/sigma_source.rs) and verifies the power structure only
// inside the ceremony (setup/mpc-setup/src/utils.rs:1447-1476, same_ratio / consistent); the prover uploads millions of records it never
// looks at.  A CRS with one bad record gives no error: it gives proofs that fail on chain.
//
//   MEMBERSHIP  tkmk_g1_check (csrc/g1check.hip) over every G1 section — xy_powers, gamma_inv_o_inst, eta_inv_li_o_inter_alpha4_kj,
//               delta_inv_li_o_prv, the three small delta tables, the six single points — each uploaded on its own: canonical coordinates,
//               on the curve, in the subgroup of order r.  Any non-zero counter fails; so does an infinity record inside xy_powers
//               ([x^a y^b]G is never infinity).  The ten G2 points are checked on the host (on_curve, g2_in_subgroup of tkmk_pairing.hpp).
//   ANCHORS     xy_powers[0] = G, xy_powers[1] = sigma_1.y, xy_powers[rs_y] = sigma_1.x (what the rkyv reader checks, here for both containers).
//   POWER STRUCTURE of xy_powers (rs_x rows of rs_y records, P[a][b] = [x^a y^b]G): with ONE grid rho of random scalars on the device
//               L_y = sum_{a, b < rs_y - 1} rho[a][b] P[a][b]      R_y = sum rho[a][b] P[a][b + 1]
//               L_x = sum_{a < rs_x - 1, b} rho[a][b] P[a][b]      R_x = sum rho[a][b] P[a + 1][b]
//               are four jobs of one tkmk_msm_multi_ex call over VIEWS of the uploaded table (bases offset by 1 resp. rs_y records; plain
//               windows, no precomputed table, nothing copied), and e(R_y, H) e(-L_y, [y]H) = 1, e(R_x, H) e(-L_x, [x]H) = 1 with H, [x]H, [y]H
//               the records 0, 8, 9 of the G2 section say P[a][b + 1] = [y]P[a][b] and P[a + 1][b] = [x]P[a][b] for every record, except with
//               probability ~ 1 / r over rho.  With the anchors that fixes the whole table.  Runs only when membership passed: an MSM
//               over points outside the subgroup proves nothing.
// SOUNDNESS rests on rho being drawn AFTER the file is fixed: the 64-bit seed comes from getrandom() at call time and expands through
// tkmk_fr_random_device.  That generator is splitmix64, which is NOT a cryptographic generator: the guarantee is against a file made
// without knowledge of the seed (64 bits of it), not against an adversary who can predict or observe the seed before fixing the file.
// TKMK_CRS_AUDIT_SEED=<n> replaces the seed in the -DTKMK_TESTING_MODE build only (as the fixed-blinding hook: the production library
// ignores it).
// OUT OF SCOPE: the structure of the gamma / eta / delta tables depends on the circuit polynomials; they get membership only.  A sharded
// prover does not audit (tkmk_prover_open_sharded does not read the variable): audit the files once before the ranks start.
#pragma once
#include <sys/random.h>

#include "tkmk_crs_load.hpp"
#include "tkmk_json.hpp"
#include "tkmk_pairing.hpp"

namespace tkmk {
namespace crs_audit {

struct SectionReport {
    std::string name;
    tkmk_g1_check_report r{};
};
struct Report {
    bool ok = false;
    std::string reason;                    // for ok == false: section, index, what is wrong
    std::vector<SectionReport> sections;   // in the order they were checked
    int g2 = -1, anchors = -1, ratio_y = -1, ratio_x = -1;   // -1: not reached (JSON null)
    double upload_s = 0, membership_s = 0, g2_s = 0, msm_s = 0, pairing_s = 0, total_s = 0;
    std::string to_json() const {
        auto esc = [](const std::string &s) {
            std::string o;
            for (char c : s) {
                if (c == '"' || c == '\\') o.push_back('\\');
                o.push_back((unsigned char)c < 0x20 ? ' ' : c);
            }
            return o;
        };
        auto tri = [](int v) { return std::string(v < 0 ? "null" : v ? "true" : "false"); };
        auto num = [](double v) {
            char b[32];
            snprintf(b, sizeof b, "%.6f", v);
            return std::string(b);
        };
        std::string d = std::string("{\"ok\": ") + (ok ? "true" : "false") + ", \"reason\": \"" + esc(reason) + "\", \"sections\": [";
        for (size_t k = 0; k < sections.size(); k++) {
            const tkmk_g1_check_report &r = sections[k].r;
            d += std::string(k ? ", " : "") + "{\"name\": \"" + sections[k].name + "\", \"points\": " + std::to_string(r.n_checked) + ", \"infinity\": " +
                 std::to_string(r.n_infinity) + ", \"noncanonical\": " + std::to_string(r.n_noncanonical) + ", \"off_curve\": " + std::to_string(r.n_off_curve) +
                 ", \"not_in_subgroup\": " + std::to_string(r.n_not_in_subgroup) + ", \"first_bad\": " +
                 (r.first_bad == UINT64_MAX ? std::string("null") : std::to_string(r.first_bad)) + "}";
        }
        d += "], \"g2\": " + tri(g2) + ", \"anchors\": " + tri(anchors) + ", \"ratio_y\": " + tri(ratio_y) + ", \"ratio_x\": " + tri(ratio_x);
        d += ", \"seconds\": {\"upload\": " + num(upload_s) + ", \"membership\": " + num(membership_s) + ", \"g2\": " + num(g2_s) + ", \"msm\": " + num(msm_s) +
             ", \"pairings\": " + num(pairing_s) + ", \"total\": " + num(total_s) + "}";
        return d + "}";
    }
};

inline SetupParams read_setup_params(const std::string &dir) {
    json::Value jp = json::read_file(dir + "/setupParams.json");
    return SetupParams{jp.at("l").as_size(),   jp.at("l_user_out").as_size(), jp.at("l_user").as_size(), jp.at("l_free").as_size(),
                       jp.at("l_D").as_size(), jp.at("m_D").as_size(),        jp.at("n").as_size(),      jp.at("s_D").as_size(),
                       jp.at("s_max").as_size()};
}

inline uint64_t draw_seed() {
#ifdef TKMK_TESTING_MODE
    if (const char *e = std::getenv("TKMK_CRS_AUDIT_SEED")) return std::strtoull(e, nullptr, 0);
#endif
    uint64_t s = 0;
    if (::getrandom(&s, sizeof s, 0) != (ssize_t)sizeof s) throw Error("getrandom failed: no entropy source for the audit's scalars");
    return s;
}

// prod_i e(p[i], q[i]) = 1 over records, as tkmk_pairing_product_is_one decides it (every point checked first)
inline bool pairing_product_is_one(const G1Affine *p, const uint8_t *const *q192, size_t n) {
    std::vector<pairing::Pair> pairs(n);
    for (size_t i = 0; i < n; i++) {
        const char *why = pairing::g1_check(p[i], pairs[i].p);
        if (*why) throw Error("crs audit: G1 operand " + std::to_string(i) + " of a pairing " + why);
        why = pairing::g2_check(q192[i], pairs[i].q);
        if (*why) throw Error("crs audit: G2 operand " + std::to_string(i) + " of a pairing " + why);
    }
    return pairing::product_is_one(pairs);
}

// The audit of one loaded payload.  Returns rep.ok; throws for what is not a verdict on the CRS (sizes that do not match setupParams.json,
// no device, a failed device call).  Everything runs on the default stream.
inline bool audit_payload(const CrsPayload &crs, const SetupParams &sp, Report &rep) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t_all = clk::now();
    rep = Report{};
    if (sp.l_D < sp.l) throw Error("Invalid setup params: l_D must be >= l.");
    const size_t m_i = sp.l_D - sp.l, rs_x = std::max(2 * sp.n, 2 * m_i), rs_y = 2 * sp.s_max;
    if (rs_x < 2 || rs_y < 2 || (uint64_t)rs_x * rs_y >= (1ull << 31)) throw Error("crs audit: xy_powers shape out of range");
    struct Sec {
        CrsPayload::Section s;
        size_t pts;
        const char *name;
    };
    const Sec secs[] = {{CrsPayload::XyPowers, rs_x * rs_y, "xy_powers"},
                        {CrsPayload::GammaInvOInst, sp.l, "gamma_inv_o_inst"},
                        {CrsPayload::EtaInvLiOInterAlpha4Kj, m_i * sp.s_max, "eta_inv_li_o_inter_alpha4_kj"},
                        {CrsPayload::DeltaInvLiOPrv, (sp.m_D - sp.l_D) * sp.s_max, "delta_inv_li_o_prv"},
                        {CrsPayload::DeltaInvAlphakXhTx, 9, "delta_inv_alphak_xh_tx"},
                        {CrsPayload::DeltaInvAlpha4XjTx, 2, "delta_inv_alpha4_xj_tx"},
                        {CrsPayload::DeltaInvAlphakYiTy, 12, "delta_inv_alphak_yi_ty"},
                        {CrsPayload::G1Singles, 6, "g1_singles"}};
    for (const Sec &s : secs)
        if (crs.points(s.s) != s.pts) throw Error(std::string("CRS section ") + s.name + " does not match setupParams.json");
    auto fail = [&](const std::string &why) {
        rep.ok = false;
        if (rep.reason.empty()) rep.reason = why;
    };
    auto finish = [&] {
        rep.total_s = since(t_all);
        return rep.ok;
    };

    // ---- membership ----
    DeviceVec<G1Affine> grid;   // xy_powers stays for the power-structure step; every other section is freed after its check
    bool members = true;
    for (const Sec &s : secs) {
        SectionReport sr;
        sr.name = s.name;
        sr.r.first_bad = UINT64_MAX;
        if (s.pts) {
            auto t0 = clk::now();
            DeviceVec<G1Affine> dev = crs.upload(s.s);
            rep.upload_s += since(t0);
            t0 = clk::now();
            check(tkmk_g1_check(dev.ptr(), TKMK_BASES_PLAIN, s.pts, 0, 0, nullptr, &sr.r, nullptr), "tkmk_g1_check");
            rep.membership_s += since(t0);
            if (s.s == CrsPayload::XyPowers) grid = std::move(dev);
        }
        const tkmk_g1_check_report &r = sr.r;
        if (r.n_noncanonical || r.n_off_curve || r.n_not_in_subgroup) {
            members = false;
            pairing::G1Aff pt;
            const char *why = r.first_bad < s.pts ? pairing::g1_check(crs.g1(s.s)[r.first_bad], pt) : "";   // the host's words for the first bad record
            fail(std::string(s.name) + "[" + std::to_string(r.first_bad) + "] " + (*why ? why : "fails the device membership check") + " (" +
                 std::to_string(r.n_noncanonical) + " not reduced, " + std::to_string(r.n_off_curve) + " off the curve, " + std::to_string(r.n_not_in_subgroup) +
                 " outside the subgroup, of " + std::to_string(s.pts) + " records)");
        } else if (s.s == CrsPayload::XyPowers && r.n_infinity) {
            members = false;
            static const uint8_t zero[96] = {};
            size_t at = 0;
            while (at < s.pts && std::memcmp(&crs.g1(s.s)[at], zero, 96) != 0) at++;
            fail("xy_powers[" + std::to_string(at) + "] is the point at infinity ([x^a y^b]G never is; " + std::to_string(r.n_infinity) + " such records)");
        }
        rep.sections.push_back(sr);
    }
    {
        const auto t0 = clk::now();
        rep.g2 = 1;
        for (int k = 0; k < 10 && rep.g2 == 1; k++) {
            g2h::Affine q;
            const char *why = pairing::g2_check(crs.bytes(CrsPayload::G2Points) + 192 * k, q);
            if (!*why && q.inf) why = "is the point at infinity";
            if (*why) rep.g2 = 0, fail("g2_points[" + std::to_string(k) + "] " + why);
        }
        rep.g2_s = since(t0);
    }
    if (!members || rep.g2 != 1) return finish();

    // ---- anchors ----
    const G1Affine *xy = crs.g1(CrsPayload::XyPowers), *singles = crs.g1(CrsPayload::G1Singles);   // G, x, y, delta, eta, lagrange_KL
    rep.anchors = 1;
    if (std::memcmp(&xy[0], &singles[0], 96) != 0) rep.anchors = 0, fail("xy_powers[0] != G");
    else if (std::memcmp(&xy[1], &singles[2], 96) != 0) rep.anchors = 0, fail("xy_powers[1] != sigma_1.y");
    else if (std::memcmp(&xy[rs_y], &singles[1], 96) != 0) rep.anchors = 0, fail("xy_powers[" + std::to_string(rs_y) + "] != sigma_1.x");

    // ---- power structure of xy_powers ----
    const size_t n = rs_x * rs_y;
    tkmk_g1_projective sums[4];
    {
        const auto t0 = clk::now();
        DeviceVec<ScalarField> rho(n);
        check(tkmk_fr_random_device(draw_seed(), 0, n, rho.ptr(), nullptr), "tkmk_fr_random_device");
        tkmk_msm_job_ex jobs[4] = {};
        for (int k = 0; k < 2; k++) {   // along Y: L_y over P[a][b], R_y over P[a][b + 1], b < rs_y - 1
            jobs[k].scalars = rho.ptr(), jobs[k].bases = grid.ptr() + k;
            jobs[k].msm_size = (int)(rs_x * (rs_y - 1));
            jobs[k].scalar_cols = jobs[k].base_cols = (uint32_t)(rs_y - 1), jobs[k].scalar_stride = jobs[k].base_stride = (uint32_t)rs_y;
            jobs[k].base_table_len = n - k;
        }
        for (int k = 0; k < 2; k++) {   // along X: L_x over P[a][b], R_x over P[a + 1][b], a < rs_x - 1
            jobs[2 + k].scalars = rho.ptr(), jobs[2 + k].bases = grid.ptr() + k * rs_y;
            jobs[2 + k].msm_size = (int)((rs_x - 1) * rs_y);
            jobs[2 + k].base_table_len = n - k * rs_y;
        }
        tkmk_msm_config cfg = tkmk_msm_default_config();
        cfg.are_scalars_on_device = cfg.are_points_on_device = true;
        check(tkmk_msm_multi_ex(jobs, 4, &cfg, TKMK_BASES_PLAIN, sums), "tkmk_msm_multi_ex");
        rep.msm_s = since(t0);
    }
    grid = DeviceVec<G1Affine>();
    {
        const auto t0 = clk::now();
        const uint8_t *g2s = crs.bytes(CrsPayload::G2Points), *H = g2s, *xH = g2s + 192 * 8, *yH = g2s + 192 * 9;
        auto holds = [&](const tkmk_g1_projective &L, const tkmk_g1_projective &Rr, const uint8_t *sH) {   // e(R, H) e(-L, [s]H) = 1
            pairing::G1Aff l;
            if (!pairing::g1_decode(projective_to_affine(L), l)) throw Error("crs audit: an MSM result is not reduced");
            const G1Affine p[2] = {projective_to_affine(Rr), pairing::g1_encode(pairing::g1_neg(l))};
            const uint8_t *q[2] = {H, sH};
            return pairing_product_is_one(p, q, 2);
        };
        rep.ratio_y = holds(sums[0], sums[1], yH) ? 1 : 0;
        rep.ratio_x = holds(sums[2], sums[3], xH) ? 1 : 0;
        rep.pairing_s = since(t0);
    }
    if (!rep.ratio_y) fail("xy_powers is not a table of powers along Y: sum rho P[a][b+1] != [y] sum rho P[a][b] for a random rho (a record is in the wrong place, or sigma_2.y is not [y]H)");
    if (!rep.ratio_x) fail("xy_powers is not a table of powers along X: sum rho P[a+1][b] != [x] sum rho P[a][b] for a random rho (a record is in the wrong place, or sigma_2.x is not [x]H)");
    rep.ok = rep.anchors == 1 && rep.ratio_y == 1 && rep.ratio_x == 1;
    return finish();
}

// <lib>/setupParams.json + <crs>/combined_sigma.{tkcrs, rkyv}; an unreadable file throws
inline bool audit_files(const std::string &lib_dir, const std::string &crs_dir, Report &rep, std::string *container = nullptr) {
    const SetupParams sp = read_setup_params(lib_dir);
    if (sp.l_D < sp.l) throw Error("Invalid setup params: l_D must be >= l.");
    const CrsPayload crs = load_combined_sigma(crs_dir, sp);
    if (container) *container = crs.container;
    return audit_payload(crs, sp, rep);
}

// TKMK_PROVER_CHECK_CRS=1 (tkmk_prover_open): unset, empty or "0" = off
inline bool requested_at_open() {
    const char *e = std::getenv("TKMK_PROVER_CHECK_CRS");
    return e && *e && std::strcmp(e, "0") != 0;
}

}  // namespace crs_audit
}  // namespace tkmk
