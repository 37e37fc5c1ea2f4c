// tkmk_crs_audit.hpp — is this reference string well formed?  The audit behind tkmk_crs_audit_files (include/tkmk_prover.h), bin/crs-check
// and the TKMK_PROVER_CHECK_CRS=1 / =2 opt-in of tkmk_prover_open, over a CrsPayload as load_combined_sigma returns it (either container).
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
//   CIRCUIT     (opt-in: `circuit` / crs-check --circuit / tkmk_crs_audit_circuit_files / TKMK_PROVER_CHECK_CRS=2; needs <lib>/subcircuitInfo.json
//               and <lib>/r1cs/)  the gamma / eta / delta tables are the only part of a reference string that ties it to THIS circuit, and every
//               binding commitment is computed from them.  Every record is s^-1 f(x, y, alpha) with s one of gamma, eta, delta and f a
//               polynomial whose coefficients come from the .r1cs files, so a random combination of a table is compared with MSMs over the
//               already verified xy_powers through one pairing product per table (audit_tables below, Sigma::gen of tkmk_setup.hpp being
//               the definition mirrored):
//                 eta          e(sum a_{l+j} b_i T[j s_max + i], [eta]H) = e(PU, [alpha]H) e(PV, [alpha^2]H) e(PW, [alpha^3]H) e(PK, [alpha^4]H)
//                 delta        the same over the private wires, without the K term, against [delta]H (an empty table is vacuously true)
//                 gamma        e(sum a_j T[j], [gamma]H) = e(PU, [alpha]H) e(PV, [alpha^2]H) e(PW, [alpha^3]H) e(PM, H)
//                 delta_small  the 9 + 2 + 12 records of the three small delta tables against differences of xy_powers records
//                 alpha_chain  e(sum d_k yi[3(k-1)], [alpha]H) = e(sum d_k yi[3k], H): with delta_small, [alpha^2]H .. [alpha^4]H are powers of alpha
//                 singles      e(sigma_1.delta, H) = e(G, [delta]H), e(sigma_1.eta, H) = e(G, [eta]H)
//               PU / PV / PW = [sum_c sum_i E[c][i] L_c(x) L_i(y)]G: the evaluation grid E (tkmk_r1cs_library_mix over per-wire weights, times b
//               through tkmk_fr_outer) -> tkmk_bintt inverse -> one MSM over the view of xy_powers.  The rank-one weights a_j b_i are
//               enough: a non-zero error table survives a random bilinear form except with probability ~ 2 / r.  The root of unity L, K, M
//               depend on is identified from the CRS first (identify_crs_root), as `prove` and `preprocess` do.  A failure says which
//               table; which record of it is for LOCATE below.
//               What this fixes: all seven G1 tables and the single points, and sigma_2 except that gamma, delta, eta are tied to the tables
//               only, not to each other.  Not covered: sigma_preprocess.rkyv, the sharded open, BN254.
//   LOCATE      (opt-in: `locate` / crs-check --locate / TKMK_CRS_AUDIT_LOCATE of tkmk_crs_audit_files_ex; never at tkmk_prover_open)  a structural
//               check that failed goes on to name the record, or says that the failure is not a record's.  Every equation above is linear
//               in its weights, so it splits into two half-checks over the SAME scalars (nothing new is drawn: the restricted sums are
//               sub-sums of the failing one, and when the lower half passes the upper half fails): host/tkmk_crs_locate.hpp descends into
//               the lower failing half with one product per level and finds the FIRST bad record; one more evaluation with that record's
//               terms set aside decides `more` (the section still fails: a further bad record, or a cause that is not a record).
//                 xy_powers    first, per failed direction, e(sigma_1.y, H) = e(G, [y]H) (resp. x): if not, sigma_2.y is not the y of
//                              sigma_1.y and nothing is searched.  Else the rectangle of relations, rows then columns, each box a view
//                              (offset pointers into rho and the table, the two-job MSM call and two-pair product of the check itself).
//                              The first failing relation has two candidate records; the one in both directions' sets is named, else
//                              the relation is.
//                 gamma        the table rows; eta / delta: the rows under the full b, then the placement columns of the row found —
//                              the last step is the equation of ONE record, an exact statement, which a record that is rightly
//                              infinity passes.  A restriction zeroes the wire weights and the a / b entries outside it (audit_tables'
//                              Cut); the uploaded table, the device library and xy_powers stay through the steps.  A step costs one
//                              evaluation of the table's equation.
//                 delta_small, alpha_chain, singles   host arithmetic: the records one at a time with unit weights.
//               Runs only where the check's own prerequisites held (membership, G2, anchors; for the tables both ratio checks).  With it
//               off, or on an honest CRS, the launches and the report's existing keys are what they were.
// A sharded prover does not audit (tkmk_prover_open_sharded does not read the variable): audit the files once before the ranks start.
#pragma once
#include <sys/random.h>

#include "tkmk_crs_load.hpp"
#include "tkmk_crs_locate.hpp"
#include "tkmk_json.hpp"
#include "tkmk_pairing.hpp"

namespace tkmk {
namespace crs_audit {

struct SectionReport {
    std::string name;
    tkmk_g1_check_report r{};
};
struct TableReport {
    std::string name;   // gamma, eta, delta, delta_small, alpha_chain, singles
    uint64_t points = 0;
    bool ok = false;
};
// what the locate pass found for one failed check: the record (index into `section`, with its row and column where the section is a
// grid), or index -1 with `what` saying why the failure is not one record's
struct Finding {
    std::string check;     // ratio_y, ratio_x, gamma, eta, delta, delta_small, alpha_chain, singles
    std::string section;   // the payload section the record is in
    int64_t index = -1, row = -1, col = -1;   // -1: JSON null
    bool more = false;     // with this record's terms removed the section still fails
    std::string what;
};
struct Report {
    bool ok = false;
    std::string reason;                    // for ok == false: section, index, what is wrong
    std::vector<SectionReport> sections;   // in the order they were checked
    int g2 = -1, anchors = -1, ratio_y = -1, ratio_x = -1;   // -1: not reached (JSON null)
    double upload_s = 0, membership_s = 0, g2_s = 0, msm_s = 0, pairing_s = 0, total_s = 0;
    int circuit = -1;                      // the table checks against the circuit: -1 not asked for or not reached, else their verdict
    std::vector<TableReport> tables;       // in the order they were checked (empty unless the table checks ran)
    double t_library_s = 0, t_grids_s = 0, t_msm_s = 0, t_pairing_s = 0;
    bool locate = false;                   // the locate pass was asked for (JSON "located": null without it)
    std::vector<Finding> located;          // in check order; empty when nothing failed, or nothing that a search may run on
    uint64_t locate_products = 0;          // pairing products spent locating
    double locate_s = 0;
    std::string to_json() const {
        using json::escape;
        const auto num = json::seconds;
        auto tri = [](int v) { return std::string(v < 0 ? "null" : v ? "true" : "false"); };
        std::string d = std::string("{\"ok\": ") + (ok ? "true" : "false") + ", \"reason\": \"" + escape(reason) + "\", \"sections\": [";
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
        d += ", \"circuit\": " + tri(circuit);
        if (circuit < 0) {
            d += ", \"tables\": null, \"table_seconds\": null";
        } else {
            d += ", \"tables\": [";
            for (size_t k = 0; k < tables.size(); k++)
                d += std::string(k ? ", " : "") + "{\"name\": \"" + tables[k].name + "\", \"points\": " + std::to_string(tables[k].points) + ", \"ok\": " +
                     (tables[k].ok ? "true" : "false") + "}";
            d += "], \"table_seconds\": {\"library\": " + num(t_library_s) + ", \"grids\": " + num(t_grids_s) + ", \"msm\": " + num(t_msm_s) + ", \"pairings\": " +
                 num(t_pairing_s) + "}";
        }
        // the locate pass: appended after every key that existed before it
        auto opt = [](int64_t v) { return v < 0 ? std::string("null") : std::to_string(v); };
        d += ", \"located\": ";
        if (!locate) {
            d += "null";
        } else {
            d += "[";
            for (size_t k = 0; k < located.size(); k++) {
                const Finding &f = located[k];
                d += std::string(k ? ", " : "") + "{\"check\": \"" + f.check + "\", \"section\": \"" + f.section + "\", \"index\": " + opt(f.index) + ", \"row\": " +
                     opt(f.row) + ", \"col\": " + opt(f.col) + ", \"more\": " + (f.more ? "true" : "false") + ", \"what\": \"" + escape(f.what) + "\"}";
            }
            d += "]";
        }
        d += ", \"locate_products\": " + std::to_string(locate_products) + ", \"locate_seconds\": " + num(locate_s);
        return d + "}";
    }
};

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

// ---- the table checks against the circuit (CIRCUIT above) ----
inline bool is_infinity(const G1Affine &p) {
    static const uint8_t zero[96] = {};
    return std::memcmp(&p, zero, 96) == 0;
}
// e(lhs, q_lhs) = prod_k e(rhs[k].first, rhs[k].second), as ONE product e(lhs, q_lhs) prod e(-rhs, q) = 1
inline bool pairing_equation(const G1Affine &lhs, const uint8_t *q_lhs, const std::vector<std::pair<G1Affine, const uint8_t *>> &rhs) {
    std::vector<G1Affine> p{lhs};
    std::vector<const uint8_t *> q{q_lhs};
    for (const auto &t : rhs) {
        pairing::G1Aff a;
        if (!pairing::g1_decode(t.first, a)) throw Error("crs audit: an MSM result is not reduced");
        p.push_back(pairing::g1_encode(pairing::g1_neg(a)));
        q.push_back(t.second);
    }
    return pairing_product_is_one(p.data(), q.data(), p.size());
}

// A restriction of a table equation for the locate pass: the table rows [r0, r1) without skip_r and, for eta / delta, the placement columns
// [c0, c1) without skip_c.  The wire weights and the b entries outside it count as zero, so both sides of the restricted equation are
// sub-sums of the full one over the same scalars.
struct Cut {
    static constexpr size_t NONE = SIZE_MAX;
    size_t r0, r1, c0, c1, skip_r = NONE, skip_c = NONE;
    bool row(size_t j) const { return j >= r0 && j < r1 && j != skip_r; }
    bool col(size_t i) const { return i >= c0 && i < c1 && i != skip_c; }
    bool empty() const { return r1 - r0 <= (size_t)(skip_r >= r0 && skip_r < r1) || c1 - c0 <= (size_t)(skip_c >= c0 && skip_c < c1); }
};

// Runs after membership, the G2 points, the anchors and both ratio checks have passed, with xy_powers (`grid`, plain records) still on
// the device.  Fills rep.tables / rep.t_*; returns whether every table holds and, if not, leaves the first failure in rep.reason.
// Throws for what is not a verdict on the CRS (an unreadable library file, a failed device call).
// locate: a table whose verdict is false is searched for its first bad record (rep.located, rep.locate_products): every table equation
// below is a callable over a Cut, the full equation being the call without one — the same launches as without `locate`.
inline bool audit_tables(const CrsPayload &crs, const SetupParams &sp, const std::string &lib_dir, DeviceVec<G1Affine> &grid, Report &rep, bool locate = false) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const size_t n = sp.n, s_max = sp.s_max, l = sp.l, l_free = sp.l_free, l_D = sp.l_D, m_D = sp.m_D, m_i = sp.m_i();
    const size_t rs_x = sp.rs_x(), rs_y = sp.rs_y(), n_prv = m_D - l_D;
    if (!is_pow2(n) || !is_pow2(s_max) || !is_pow2(m_i) || (l_free && !is_pow2(l_free))) throw Error("crs audit: n, s_max, m_I and l_free must be powers of two");
    if (s_max < 4 || m_D < l_D || l_free > l || n + 2 >= rs_x || m_i + 1 >= rs_x) throw Error("crs audit: setup parameters out of range for the table checks");
    if (grid.len() != rs_x * rs_y) throw Error("crs audit: the table checks need xy_powers on the device");
    rep.tables.clear();
    // what = "<section>: <what a failure means>"
    auto verdict = [&](const char *name, uint64_t points, bool ok, const std::string &what) {
        rep.tables.push_back(TableReport{name, points, ok});
        const size_t cut = what.find(": ");
        if (!ok && rep.reason.empty())
            rep.reason = std::string("table ") + name + ": a record of " + what.substr(0, cut) + " is not what the circuit of " + lib_dir + " and sigma_2 determine" +
                         what.substr(cut);
        return ok;
    };

    // ---- the library: CSR on the device, and who owns each flattened wire ----
    auto t0 = clk::now();
    const SubcircuitLibrary library = SubcircuitLibrary::read(lib_dir, sp);
    const std::vector<SubcircuitR1CS> &r1cs = library.r1cs;
    const size_t K = library.infos.size();
    if (K == 0) throw Error("subcircuitInfo.json names no subcircuit");
    const std::vector<std::vector<uint8_t>> own = flat_wire_owners(library.infos, r1cs, m_D);
    const DeviceLibrary dlib = DeviceLibrary::create(r1cs);
    std::vector<size_t> w_off(K + 1, 0);
    for (size_t k = 0; k < K; k++) w_off[k + 1] = w_off[k] + r1cs[k].n_wires;
    rep.t_library_s = since(t0);

    // ---- the root of unity L_i, K_j, M_j are taken over: the one the CRS was made under ----
    const G1Affine *xy = crs.g1(CrsPayload::XyPowers), *singles = crs.g1(CrsPayload::G1Singles);
    try {
        identify_crs_root(grid.ptr(), TKMK_BASES_PLAIN, singles[5], sp, true);
    } catch (const Error &e) {
        if (std::strncmp(e.what(), "the reference string's lagrange_KL", 34) != 0) throw;
        if (rep.reason.empty()) rep.reason = std::string("the table checks need the root of unity the CRS was made under: ") + e.what();
        return false;
    }
    init_ntt_domain_for_size(std::max(std::max(n, m_i), std::max(l_free, (size_t)1)) * s_max);

    // ---- the scalars: a per flattened wire, b per placement column, 23 + 3 for the small tables, drawn after the file was fixed ----
    t0 = clk::now();
    const size_t n_rand = m_D + s_max + 26;
    DeviceVec<ScalarField> rnd(n_rand);
    check(tkmk_fr_random_device(draw_seed(), (uint64_t)rs_x * rs_y, n_rand, rnd.ptr(), nullptr), "tkmk_fr_random_device");
    const std::vector<ScalarField> rnd_h = rnd.to_host();
    const ScalarField *a_dev = rnd.ptr(), *b_dev = rnd.ptr() + m_D;
    const ScalarField *a = rnd_h.data(), *b = rnd_h.data() + m_D, *c_small = rnd_h.data() + m_D + s_max, *d_chain = c_small + 23;

    // per-kind weights of the three wire ranges, and the gamma table's column of each wire
    enum { W_GAMMA = 0, W_ETA, W_DELTA };
    auto g_of = [&](size_t f) { return f < sp.l_user_out ? 0 : f < sp.l_user ? 1 : f < l_free ? 2 : 3; };
    std::vector<ScalarField> wt_h[3];
    std::vector<uint8_t> col_h(w_off[K] ? w_off[K] : 1, 0);
    for (auto &v : wt_h) v.assign(w_off[K] ? w_off[K] : 1, ScalarField{});
    for (size_t k = 0; k < K; k++)
        for (size_t j = 0; j < r1cs[k].n_wires; j++) {
            const size_t f = library.infos[k].flattenMap[j];
            if (f >= m_D) throw Error("subcircuitInfo.json: flattenMap entry outside the global wire range");
            if (f < l) col_h[w_off[k] + j] = (uint8_t)g_of(f);
            if (own[k][j]) wt_h[f < l ? W_GAMMA : f < l_D ? W_ETA : W_DELTA][w_off[k] + j] = a[f];
        }
    DeviceVec<ScalarField> wt_dev[3] = {DeviceVec<ScalarField>::from_host(wt_h[0]), DeviceVec<ScalarField>::from_host(wt_h[1]), DeviceVec<ScalarField>::from_host(wt_h[2])};
    DeviceVec<uint8_t> col_dev = DeviceVec<uint8_t>::from_host(col_h);
    auto kind_ptrs = [&](const ScalarField *base) {
        std::vector<const tkmk_fr *> p(K);
        for (size_t k = 0; k < K; k++) p[k] = base + w_off[k];
        return p;
    };
    std::vector<const uint8_t *> col_ptrs(K);
    for (size_t k = 0; k < K; k++) col_ptrs[k] = col_dev.ptr() + w_off[k];
    rep.t_grids_s += since(t0);
    // the same scalars under a Cut (locate pass): the weights of the wires whose table row the cut leaves out, and the entries of a / b it
    // leaves out, are zero; nothing new is drawn.  first = the flattened wire of table row 0.
    auto cut_weights = [&](int range, size_t first, const Cut &cut) {
        std::vector<ScalarField> v = wt_h[range];
        for (size_t k = 0; k < K; k++)
            for (size_t j = 0; j < r1cs[k].n_wires; j++) {
                const size_t f = library.infos[k].flattenMap[j];
                if (f < first || !cut.row(f - first)) v[w_off[k] + j] = ScalarField{};
            }
        return DeviceVec<ScalarField>::from_host(v);
    };
    auto cut_a = [&](size_t first, size_t rows, const Cut &cut) {
        std::vector<ScalarField> v(rows, ScalarField{});
        for (size_t j = 0; j < rows; j++)
            if (cut.row(j)) v[j] = a[first + j];
        return DeviceVec<ScalarField>::from_host(v);
    };
    auto cut_b = [&](const Cut &cut) {
        std::vector<ScalarField> v(s_max, ScalarField{});
        for (size_t i = 0; i < s_max; i++)
            if (cut.col(i)) v[i] = b[i];
        return DeviceVec<ScalarField>::from_host(v);
    };
    double t_locate_sink = 0;   // the times of restricted evaluations stay out of table_seconds (rep.locate_s has them as a whole)
    auto times = [&](double &field, const Cut *cut) -> double & { return cut ? t_locate_sink : field; };
    auto add_finding = [&](const char *check, const std::string &section, int64_t index, int64_t row, int64_t col, bool more, const std::string &what) {
        Finding f;
        f.check = check, f.section = section, f.index = index, f.row = row, f.col = col, f.more = more, f.what = what;
        rep.located.push_back(f);
    };
    const std::string not_determined = " is not the record that the circuit of " + lib_dir + " and sigma_2 determine";
    auto more_words = [](bool more, const char *systemic) {
        return more ? std::string("; with it set aside the table still fails: at least one more record is wrong, or the cause is not a record (") + systemic + ")"
                    : std::string("; every other record of the table satisfies the equation");
    };

    const uint8_t *g2s = crs.bytes(CrsPayload::G2Points);
    auto g2 = [&](int k) { return g2s + 192 * k; };   // 0 H, 1..4 [alpha^k]H, 5 [gamma]H, 6 [delta]H, 7 [eta]H, 8 [x]H, 9 [y]H
    tkmk_msm_config cfg = tkmk_msm_default_config();
    cfg.are_scalars_on_device = cfg.are_points_on_device = true;
    // [sum coeff[h][i] x^h y^i]G over the xs x s_max corner of xy_powers
    auto corner_job = [&](const DeviceVec<ScalarField> &coeffs, size_t xs) {
        tkmk_msm_job_ex j{};
        j.scalars = coeffs.ptr(), j.bases = grid.ptr(), j.msm_size = (int)(xs * s_max);
        j.scalar_cols = j.scalar_stride = j.base_cols = (uint32_t)s_max, j.base_stride = (uint32_t)rs_y;
        j.base_table_len = rs_x * rs_y;
        return j;
    };
    auto coefficients = [&](const DeviceVec<ScalarField> &evals, size_t xs, size_t ys) {
        DeviceVec<ScalarField> out(xs * ys);
        check(tkmk_bintt(evals.ptr(), xs, ys, TKMK_NTT_INVERSE, nullptr, nullptr, true, nullptr, out.ptr()), "tkmk_bintt");
        return out;
    };
    bool all = true;

    // ---- eta and delta: T[j s_max + i] = s^-1 L_i(y) (o_{first + j}(x) [+ alpha^4 K_j(x)]) ----
    auto outer_table = [&](const char *name, const char *what, CrsPayload::Section sec, int range, size_t first, size_t rows, bool with_k, int g2_s) {
        if (rows == 0) return verdict(name, 0, true, what);   // vacuously true
        DeviceVec<G1Affine> table;   // uploaded by the first evaluation; stays through a search
        // the table's equation over a restriction (nullptr: all of it): an empty restriction holds without being evaluated
        auto holds = [&](const Cut *cut) {
            if (cut && cut->empty()) return true;
            auto t1 = clk::now();
            DeviceVec<ScalarField> w_cut, a_cut, b_cut;
            if (cut) w_cut = cut_weights(range, first, *cut), a_cut = cut_a(first, rows, *cut), b_cut = cut_b(*cut);
            const ScalarField *a_use = cut ? a_cut.ptr() : a_dev + first, *b_use = cut ? b_cut.ptr() : b_dev;
            const std::vector<const tkmk_fr *> wp = kind_ptrs(cut ? w_cut.ptr() : wt_dev[range].ptr());
            DeviceVec<ScalarField> col[3] = {DeviceVec<ScalarField>(n), DeviceVec<ScalarField>(n), DeviceVec<ScalarField>(n)};
            check(tkmk_r1cs_library_mix(dlib.get(), wp.data(), nullptr, (uint32_t)n, 1, 1, col[0].ptr(), col[1].ptr(), col[2].ptr(), nullptr), "tkmk_r1cs_library_mix");
            DeviceVec<ScalarField> coeff[3];
            for (int m = 0; m < 3; m++) {
                DeviceVec<ScalarField> ev(n * s_max);
                check(tkmk_fr_outer(col[m].ptr(), (uint32_t)n, b_use, (uint32_t)s_max, (uint32_t)s_max, ev.ptr(), nullptr), "tkmk_fr_outer");
                coeff[m] = coefficients(ev, n, s_max);
            }
            DeviceVec<ScalarField> ab(rows * s_max), k_coeff;   // a_{first + j} b_i: the combination of the table, and the grid of the K term
            check(tkmk_fr_outer(a_use, (uint32_t)rows, b_use, (uint32_t)s_max, (uint32_t)s_max, ab.ptr(), nullptr), "tkmk_fr_outer");
            if (with_k) k_coeff = coefficients(ab, rows, s_max);
            check(tkmk_device_synchronize(), "synchronize");
            times(rep.t_grids_s, cut) += since(t1);
            t1 = clk::now();
            if (!table.len()) table = crs.upload(sec);
            tkmk_msm_job_ex jobs[5] = {};
            jobs[0].scalars = ab.ptr(), jobs[0].bases = table.ptr(), jobs[0].msm_size = (int)(rows * s_max), jobs[0].base_table_len = rows * s_max;
            for (int m = 0; m < 3; m++) jobs[1 + m] = corner_job(coeff[m], n);
            if (with_k) jobs[4] = corner_job(k_coeff, rows);
            tkmk_g1_projective sums[5];
            check(tkmk_msm_multi_ex(jobs, with_k ? 5 : 4, &cfg, TKMK_BASES_PLAIN, sums), "tkmk_msm_multi_ex");
            times(rep.t_msm_s, cut) += since(t1);
            t1 = clk::now();
            std::vector<std::pair<G1Affine, const uint8_t *>> rhs;
            for (int m = 0; m < 3; m++) rhs.push_back({projective_to_affine(sums[1 + m]), g2(1 + m)});
            if (with_k) rhs.push_back({projective_to_affine(sums[4]), g2(4)});
            const bool ok = pairing_equation(projective_to_affine(sums[0]), g2(g2_s), rhs);
            times(rep.t_pairing_s, cut) += since(t1);
            if (cut) rep.locate_products++;
            return ok;
        };
        const bool ok = holds(nullptr);
        verdict(name, rows * s_max, ok, what);
        if (!ok && locate) {
            // rows j under the full b, then the columns i of the row found: the last step is the equation of T[j s_max + i] alone (weight
            // a_j b_i != 0), an exact statement.  A record that is rightly infinity has a vanishing right side and passes it.
            const auto t1 = clk::now();
            size_t calls = 0;
            const crs_locate::Cell at = crs_locate::first_bad_cell(rows, s_max, [&](size_t r0, size_t r1, size_t c0, size_t c1) {
                const Cut cut{r0, r1, c0, c1};
                return !holds(&cut);
            }, calls);
            const Cut no_row{0, rows, 0, s_max, at.row, Cut::NONE}, no_col{at.row, at.row + 1, 0, s_max, Cut::NONE, at.col};
            const bool more = !holds(&no_row) || !holds(&no_col);
            const std::string section = std::string(what).substr(0, std::string(what).find(": "));
            const size_t index = at.row * s_max + at.col;
            add_finding(name, section, (int64_t)index, (int64_t)at.row, (int64_t)at.col, more,
                        section + "[" + std::to_string(index) + "] (wire " + std::to_string(first + at.row) + ", placement column " + std::to_string(at.col) + ")" +
                            not_determined + more_words(more, (std::string("a CRS made for another library, or a wrong sigma_2.") + name).c_str()));
            rep.locate_s += since(t1);
        }
        return ok;
    };

    // ---- gamma: T[j] = gamma^-1 (L_{g(j)}(y) o_j(x) + [j < l_free] M_j(x)) ----
    auto gamma_table = [&]() {
        const char *what = "gamma_inv_o_inst: a wrong or misplaced record, a CRS made for another library, or a wrong sigma_2.gamma";
        if (l == 0) return verdict("gamma", 0, true, what);
        DeviceVec<G1Affine> table;   // uploaded by the first evaluation; stays through a search
        auto holds = [&](const Cut *cut) {   // the rows of a Cut are table rows j = flattened wires; its columns are not used
            if (cut && cut->empty()) return true;
            auto t1 = clk::now();
            DeviceVec<ScalarField> w_cut, a_cut;
            if (cut) w_cut = cut_weights(W_GAMMA, 0, *cut), a_cut = cut_a(0, l, *cut);
            const ScalarField *a_use = cut ? a_cut.ptr() : a_dev;
            const std::vector<const tkmk_fr *> wp = kind_ptrs(cut ? w_cut.ptr() : wt_dev[W_GAMMA].ptr());
            DeviceVec<ScalarField> coeff[3];
            {
                DeviceVec<ScalarField> ev[3] = {DeviceVec<ScalarField>(n * s_max), DeviceVec<ScalarField>(n * s_max), DeviceVec<ScalarField>(n * s_max)};
                for (auto &e : ev) check(tkmk_memset(e.ptr(), 0, n * s_max * sizeof(ScalarField)), "tkmk_memset");
                check(tkmk_r1cs_library_mix(dlib.get(), wp.data(), col_ptrs.data(), (uint32_t)n, 4, (uint32_t)s_max, ev[0].ptr(), ev[1].ptr(), ev[2].ptr(), nullptr),
                      "tkmk_r1cs_library_mix");
                for (int m = 0; m < 3; m++) coeff[m] = coefficients(ev[m], n, s_max);
            }
            DeviceVec<ScalarField> m_coeff;
            if (l_free) {
                m_coeff = DeviceVec<ScalarField>(l_free);
                check(tkmk_bintt(a_use, l_free, 1, TKMK_NTT_INVERSE, nullptr, nullptr, true, nullptr, m_coeff.ptr()), "tkmk_bintt");
            }
            check(tkmk_device_synchronize(), "synchronize");
            times(rep.t_grids_s, cut) += since(t1);
            t1 = clk::now();
            if (!table.len()) table = crs.upload(CrsPayload::GammaInvOInst);
            tkmk_msm_job_ex jobs[5] = {};
            jobs[0].scalars = a_use, jobs[0].bases = table.ptr(), jobs[0].msm_size = (int)l, jobs[0].base_table_len = l;
            for (int m = 0; m < 3; m++) jobs[1 + m] = corner_job(coeff[m], n);
            if (l_free) {   // column 0 of xy_powers: [x^h]G
                jobs[4].scalars = m_coeff.ptr(), jobs[4].bases = grid.ptr(), jobs[4].msm_size = (int)l_free;
                jobs[4].base_cols = 1, jobs[4].base_stride = (uint32_t)rs_y, jobs[4].scalar_cols = 1, jobs[4].scalar_stride = 1;
                jobs[4].base_table_len = rs_x * rs_y;
            }
            tkmk_g1_projective sums[5];
            check(tkmk_msm_multi_ex(jobs, l_free ? 5 : 4, &cfg, TKMK_BASES_PLAIN, sums), "tkmk_msm_multi_ex");
            times(rep.t_msm_s, cut) += since(t1);
            t1 = clk::now();
            std::vector<std::pair<G1Affine, const uint8_t *>> rhs;
            for (int m = 0; m < 3; m++) rhs.push_back({projective_to_affine(sums[1 + m]), g2(1 + m)});
            if (l_free) rhs.push_back({projective_to_affine(sums[4]), g2(0)});
            const bool ok = pairing_equation(projective_to_affine(sums[0]), g2(5), rhs);
            times(rep.t_pairing_s, cut) += since(t1);
            if (cut) rep.locate_products++;
            return ok;
        };
        const bool ok = holds(nullptr);
        verdict("gamma", l, ok, what);
        if (!ok && locate) {
            const auto t1 = clk::now();
            size_t calls = 0;
            const size_t at = crs_locate::first_bad(l, [&](size_t lo, size_t hi) {
                const Cut cut{lo, hi, 0, 1};
                return !holds(&cut);
            }, calls);
            const Cut rest{0, l, 0, 1, at, Cut::NONE};
            const bool more = !holds(&rest);
            add_finding("gamma", "gamma_inv_o_inst", (int64_t)at, -1, -1, more,
                        "gamma_inv_o_inst[" + std::to_string(at) + "]" + not_determined + more_words(more, "a CRS made for another library, or a wrong sigma_2.gamma"));
            rep.locate_s += since(t1);
        }
        return ok;
    };
    all &= gamma_table();
    all &= outer_table("eta", "eta_inv_li_o_inter_alpha4_kj: a wrong or misplaced record, a CRS made for another library, or a wrong sigma_2.eta",
                       CrsPayload::EtaInvLiOInterAlpha4Kj, W_ETA, l, m_i, true, 7);
    all &= outer_table("delta", "delta_inv_li_o_prv: a wrong or misplaced record, a CRS made for another library, or a wrong sigma_2.delta",
                       CrsPayload::DeltaInvLiOPrv, W_DELTA, l_D, n_prv, false, 6);

    // ---- the small delta tables, the alpha chain and the single points: host arithmetic ----
    t0 = clk::now();
    const double located_before = rep.locate_s;   // what the locate pass spends below is its own time, not the tables'
    auto pt = [&](const G1Affine &rec) {
        pairing::G1Aff p;
        if (!pairing::g1_decode(rec, p)) throw Error("crs audit: a record that passed membership is not reduced");
        return p;
    };
    const G1Affine *xh = crs.g1(CrsPayload::DeltaInvAlphakXhTx), *xj = crs.g1(CrsPayload::DeltaInvAlpha4XjTx), *yi = crs.g1(CrsPayload::DeltaInvAlphakYiTy);
    {
        bool none_inf = true;
        for (int k = 0; k < 9; k++) none_inf &= !is_infinity(xh[k]);
        for (int k = 0; k < 2; k++) none_inf &= !is_infinity(xj[k]);
        for (int k = 0; k < 12; k++) none_inf &= !is_infinity(yi[k]);
        bool ok = none_inf;
        if (ok) {
            // c: [0, 9) for xh, [9, 11) for xj, [11, 23) for yi
            std::vector<std::pair<ScalarField, pairing::G1Aff>> lhs;
            for (int k = 0; k < 9; k++) lhs.push_back({c_small[k], pt(xh[k])});
            for (int k = 0; k < 2; k++) lhs.push_back({c_small[9 + k], pt(xj[k])});
            for (int k = 0; k < 12; k++) lhs.push_back({c_small[11 + k], pt(yi[k])});
            auto diff = [&](std::vector<std::pair<ScalarField, pairing::G1Aff>> &t, const ScalarField &c, size_t hi, size_t lo) {   // c (xy[hi] - xy[lo])
                t.push_back({c, pt(xy[hi])});
                t.push_back({fr_neg(c), pt(xy[lo])});
            };
            std::vector<std::pair<G1Affine, const uint8_t *>> rhs;
            for (int k = 1; k <= 4; k++) {
                std::vector<std::pair<ScalarField, pairing::G1Aff>> t;
                if (k <= 3)
                    for (size_t h = 0; h < 3; h++) diff(t, c_small[3 * (k - 1) + h], (n + h) * rs_y, h * rs_y);        // x^h (x^n - 1)
                else
                    for (size_t j = 0; j < 2; j++) diff(t, c_small[9 + j], (m_i + j) * rs_y, j * rs_y);                  // x^j (x^m_I - 1)
                for (size_t i = 0; i < 3; i++) diff(t, c_small[11 + 3 * (k - 1) + i], s_max + i, i);                     // y^i (y^s_max - 1)
                rhs.push_back({pairing::g1_encode(pairing::g1_lincomb(t)), g2(k)});
            }
            ok = pairing_equation(pairing::g1_encode(pairing::g1_lincomb(lhs)), g2(6), rhs);
        }
        all &= verdict("delta_small", 23, ok,
                       none_inf ? "delta_inv_alphak_xh_tx / delta_inv_alpha4_xj_tx / delta_inv_alphak_yi_ty: a wrong or misplaced record, or a wrong sigma_2.delta or sigma_2.alpha^k"
                                : "delta_inv_alphak_xh_tx / delta_inv_alpha4_xj_tx / delta_inv_alphak_yi_ty: one is the point at infinity, which delta^-1 alpha^k t(x) never is");
        if (!ok && locate) {   // the 23 records one at a time, unit weights: e(record, [delta]H) = e(xy[hi] - xy[lo], [alpha^k]H)
            const auto t1 = clk::now();
            const ScalarField one = fr_one();
            struct Small {
                const char *section;
                const G1Affine *rec;
                size_t index, hi, lo;
                int k;
            };
            std::vector<Small> recs;
            for (int k = 1; k <= 3; k++)
                for (size_t h = 0; h < 3; h++) recs.push_back({"delta_inv_alphak_xh_tx", xh, 3 * (size_t)(k - 1) + h, (n + h) * rs_y, h * rs_y, k});
            for (size_t j = 0; j < 2; j++) recs.push_back({"delta_inv_alpha4_xj_tx", xj, j, (m_i + j) * rs_y, j * rs_y, 4});
            for (int k = 1; k <= 4; k++)
                for (size_t i = 0; i < 3; i++) recs.push_back({"delta_inv_alphak_yi_ty", yi, 3 * (size_t)(k - 1) + i, s_max + i, i, k});
            const Small *first_bad = nullptr;
            size_t n_bad = 0;
            for (const Small &s : recs) {
                bool good = !is_infinity(s.rec[s.index]);
                if (good) {
                    const pairing::G1Aff d = pairing::g1_lincomb({{one, pt(xy[s.hi])}, {fr_neg(one), pt(xy[s.lo])}});
                    good = pairing_equation(s.rec[s.index], g2(6), {{pairing::g1_encode(d), g2(s.k)}});
                    rep.locate_products++;
                }
                if (!good && !n_bad++) first_bad = &s;
            }
            if (first_bad)
                add_finding("delta_small", first_bad->section, (int64_t)first_bad->index, -1, -1, n_bad > 1,
                            std::string(first_bad->section) + "[" + std::to_string(first_bad->index) + "] is not [delta^-1 alpha^" + std::to_string(first_bad->k) +
                                "] (xy_powers[" + std::to_string(first_bad->hi) + "] - xy_powers[" + std::to_string(first_bad->lo) + "]) for the delta and alpha^" +
                                std::to_string(first_bad->k) + " of sigma_2" +
                                (n_bad > 1 ? "; " + std::to_string(n_bad - 1) + " more of the 23 records fail as well (records in each other's place, or a wrong sigma_2.delta or sigma_2.alpha^k)"
                                           : std::string("; the other 22 records hold")));
            rep.locate_s += since(t1);
        }
    }
    {
        std::vector<std::pair<ScalarField, pairing::G1Aff>> lo, hi;
        for (int k = 1; k <= 3; k++) lo.push_back({d_chain[k - 1], pt(yi[3 * (k - 1)])}), hi.push_back({d_chain[k - 1], pt(yi[3 * k])});
        const bool ok = pairing_equation(pairing::g1_encode(pairing::g1_lincomb(lo)), g2(1), {{pairing::g1_encode(pairing::g1_lincomb(hi)), g2(0)}});
        all &= verdict("alpha_chain", 4, ok, "delta_inv_alphak_yi_ty along alpha: yi[3k] is not [alpha] yi[3(k-1)], so a record is misplaced or sigma_2.alpha .. alpha4 are not powers of one alpha");
        if (!ok && locate) {   // the three links one at a time: e(yi[3(k-1)], [alpha]H) = e(yi[3k], H); the record named is the link's target
            const auto t1 = clk::now();
            int first_bad = 0, n_bad = 0;
            for (int k = 1; k <= 3; k++) {
                rep.locate_products++;
                if (!pairing_equation(yi[3 * (k - 1)], g2(1), {{yi[3 * k], g2(0)}}) && !n_bad++) first_bad = k;
            }
            if (n_bad)
                add_finding("alpha_chain", "delta_inv_alphak_yi_ty", 3 * first_bad, -1, -1, n_bad > 1,
                            "delta_inv_alphak_yi_ty[" + std::to_string(3 * first_bad) + "] is not [alpha] delta_inv_alphak_yi_ty[" + std::to_string(3 * (first_bad - 1)) +
                                "] for the alpha of sigma_2" + (n_bad > 1 ? "; another link of the chain fails as well" : "; the other two links hold"));
            rep.locate_s += since(t1);
        }
    }
    {
        const bool ok = pairing_equation(singles[3], g2(0), {{singles[0], g2(6)}}) && pairing_equation(singles[4], g2(0), {{singles[0], g2(7)}});
        all &= verdict("singles", 2, ok, "sigma_1.delta / sigma_1.eta: they are not [delta]G and [eta]G for the delta and eta of sigma_2");
        if (!ok && locate) {
            const auto t1 = clk::now();
            const bool bad_delta = !pairing_equation(singles[3], g2(0), {{singles[0], g2(6)}}), bad_eta = !pairing_equation(singles[4], g2(0), {{singles[0], g2(7)}});
            rep.locate_products += 2;
            if (bad_delta || bad_eta) {
                const char *s = bad_delta ? "delta" : "eta";
                add_finding("singles", "g1_singles", bad_delta ? 3 : 4, -1, -1, bad_delta && bad_eta,
                            std::string("sigma_1.") + s + " (g1_singles[" + (bad_delta ? "3" : "4") + "]) is not [" + s + "]G for the " + s + " of sigma_2" +
                                (bad_delta && bad_eta ? "; sigma_1.eta is not [eta]G either" : ""));
            }
            rep.locate_s += since(t1);
        }
    }
    rep.t_pairing_s += since(t0) - (rep.locate_s - located_before);
    return all;
}

// The audit of one loaded payload.  Returns rep.ok; throws for what is not a verdict on the CRS (sizes that do not match setupParams.json,
// no device, a failed device call).  Everything runs on the default stream.
// locate: a structural check that fails is followed by the search for the record (LOCATE in the head of this file); with it off, or
// on an honest CRS, nothing else runs than without it.
inline bool audit_payload(const CrsPayload &crs, const SetupParams &sp, Report &rep, bool circuit = false, const std::string &lib_dir = std::string(),
                          bool locate = false) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    const auto t_all = clk::now();
    rep = Report{};
    rep.locate = locate;
    validate_setup_shape(sp);
    const size_t rs_x = sp.rs_x(), rs_y = sp.rs_y();
    if (rs_x < 2 || rs_y < 2 || (uint64_t)rs_x * rs_y >= (1ull << 31)) throw Error("crs audit: xy_powers shape out of range");
    check_crs_sections(crs, sp);
    auto fail = [&](const std::string &why) {
        rep.ok = false;
        if (rep.reason.empty()) rep.reason = why;
    };
    auto finish = [&] {
        if (!rep.located.empty() && !rep.reason.empty()) rep.reason += " Located: " + rep.located[0].what;
        rep.total_s = since(t_all);
        return rep.ok;
    };

    // ---- membership ----
    DeviceVec<G1Affine> grid;   // xy_powers stays for the power-structure step; every other section is freed after its check
    bool members = true;
    for (const CrsSectionSpec &s : crs_sections()) {
        const size_t pts = s.points(sp);
        SectionReport sr;
        sr.name = s.name;
        sr.r.first_bad = UINT64_MAX;
        if (pts) {
            auto t0 = clk::now();
            DeviceVec<G1Affine> dev = crs.upload(s.s);
            rep.upload_s += since(t0);
            t0 = clk::now();
            check(tkmk_g1_check(dev.ptr(), TKMK_BASES_PLAIN, pts, 0, 0, nullptr, &sr.r, nullptr), "tkmk_g1_check");
            rep.membership_s += since(t0);
            if (s.s == CrsPayload::XyPowers) grid = std::move(dev);
        }
        const tkmk_g1_check_report &r = sr.r;
        if (r.n_noncanonical || r.n_off_curve || r.n_not_in_subgroup) {
            members = false;
            pairing::G1Aff pt;
            const char *why = r.first_bad < pts ? pairing::g1_check(crs.g1(s.s)[r.first_bad], pt) : "";   // the host's words for the first bad record
            fail(std::string(s.name) + "[" + std::to_string(r.first_bad) + "] " + (*why ? why : "fails the device membership check") + " (" +
                 std::to_string(r.n_noncanonical) + " not reduced, " + std::to_string(r.n_off_curve) + " off the curve, " + std::to_string(r.n_not_in_subgroup) +
                 " outside the subgroup, of " + std::to_string(pts) + " records)");
        } else if (s.s == CrsPayload::XyPowers && r.n_infinity) {
            members = false;
            static const uint8_t zero[96] = {};
            size_t at = 0;
            while (at < pts && std::memcmp(&crs.g1(s.s)[at], zero, 96) != 0) at++;
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
    DeviceVec<ScalarField> rho;   // a search reuses it; without `locate` it is freed with the MSMs, as it was
    {
        const auto t0 = clk::now();
        rho = DeviceVec<ScalarField>(n);
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
    if (!locate) rho = DeviceVec<ScalarField>();
    if (!circuit && !locate) grid = DeviceVec<G1Affine>();   // the table checks, and a search, read xy_powers again
    const uint8_t *g2s = crs.bytes(CrsPayload::G2Points), *H = g2s, *xH = g2s + 192 * 8, *yH = g2s + 192 * 9;
    auto holds = [&](const tkmk_g1_projective &L, const tkmk_g1_projective &Rr, const uint8_t *sH) {   // e(R, H) e(-L, [s]H) = 1
        pairing::G1Aff l;
        if (!pairing::g1_decode(projective_to_affine(L), l)) throw Error("crs audit: an MSM result is not reduced");
        const G1Affine p[2] = {projective_to_affine(Rr), pairing::g1_encode(pairing::g1_neg(l))};
        const uint8_t *q[2] = {H, sH};
        return pairing_product_is_one(p, q, 2);
    };
    {
        const auto t0 = clk::now();
        rep.ratio_y = holds(sums[0], sums[1], yH) ? 1 : 0;
        rep.ratio_x = holds(sums[2], sums[3], xH) ? 1 : 0;
        rep.pairing_s = since(t0);
    }
    if (locate && rep.anchors == 1 && (!rep.ratio_y || !rep.ratio_x)) {
        // ---- LOCATE: which record of xy_powers?  (membership, G2 and the anchors are clean here) ----
        const auto t0 = clk::now();
        tkmk_msm_config cfg = tkmk_msm_default_config();
        cfg.are_scalars_on_device = cfg.are_points_on_device = true;
        // direction d: 0 along Y (relation (a, b): P[a][b + 1] = [y]P[a][b], b < rs_y - 1), 1 along X (P[a + 1][b] = [x]P[a][b], a < rs_x - 1).
        // The relations of a box, weighted by `weights` (rho or a copy of it): the two-job call and the two-pair product of the check
        // itself over VIEWS of rho and of the table, offset to the box's corner — nothing is copied.
        auto box_fails = [&](int d, const ScalarField *weights, size_t a0, size_t a1, size_t b0, size_t b1) {
            const size_t corner = a0 * rs_y + b0, step = d ? rs_y : 1;
            tkmk_msm_job_ex jobs[2] = {};
            for (int k = 0; k < 2; k++) {
                jobs[k].scalars = weights + corner, jobs[k].bases = grid.ptr() + corner + k * step;
                jobs[k].msm_size = (int)((a1 - a0) * (b1 - b0));
                jobs[k].scalar_cols = jobs[k].base_cols = (uint32_t)(b1 - b0), jobs[k].scalar_stride = jobs[k].base_stride = (uint32_t)rs_y;
                jobs[k].base_table_len = n - corner - k * step;
            }
            tkmk_g1_projective s2[2];
            check(tkmk_msm_multi_ex(jobs, 2, &cfg, TKMK_BASES_PLAIN, s2), "tkmk_msm_multi_ex");
            rep.locate_products++;
            return !holds(s2[0], s2[1], d ? xH : yH);
        };
        const size_t rel_rows[2] = {rs_x, rs_x - 1}, rel_cols[2] = {rs_y - 1, rs_y};
        const char *coord[2] = {"y", "x"}, *checks[2] = {"ratio_y", "ratio_x"};
        const int failed[2] = {!rep.ratio_y, !rep.ratio_x};
        bool systemic[2] = {false, false}, found[2] = {false, false};
        size_t source[2] = {0, 0};   // the first failing relation of a direction, as the flat index of its source record
        for (int d = 0; d < 2; d++) {
            if (!failed[d]) continue;
            // the anchors fix xy[0] = G, xy[1] = sigma_1.y, xy[rs_y] = sigma_1.x: does sigma_2 carry the same y (x) as sigma_1?
            rep.locate_products++;
            if (!pairing_equation(singles[d ? 1 : 2], H, {{singles[0], d ? xH : yH}})) {
                systemic[d] = true;
                continue;
            }
            size_t calls = 0;
            const crs_locate::Cell at = crs_locate::first_bad_cell(rel_rows[d], rel_cols[d], [&](size_t a0, size_t a1, size_t b0, size_t b1) {
                return box_fails(d, rho.ptr(), a0, a1, b0, b1);
            }, calls);
            found[d] = true, source[d] = at.row * rs_y + at.col;
        }
        // the record both first failing relations touch, if both directions have one; else the relation itself
        const size_t record = found[0] && found[1] ? crs_locate::meet(source[0], source[1], rs_y) : SIZE_MAX;
        bool more = false;
        if (found[0] || found[1]) {
            // the checks once more with the relations set aside: those touching the record (two per direction at most), or the one relation
            DeviceVec<ScalarField> rest = rho.clone();
            for (int d = 0; d < 2; d++) {
                if (!found[d]) continue;
                const size_t step = d ? rs_y : 1;
                size_t drop[2], n_drop = 0;
                if (record == SIZE_MAX) {
                    drop[n_drop++] = source[d];
                } else {
                    const size_t a = record / rs_y, b = record % rs_y;
                    if (d ? a + 1 < rs_x : b + 1 < rs_y) drop[n_drop++] = record;          // the record as a source
                    if (d ? a > 0 : b > 0) drop[n_drop++] = record - step;                  // ... and as a target
                }
                for (size_t k = 0; k < n_drop; k++) check(tkmk_memset(rest.ptr() + drop[k], 0, sizeof(ScalarField)), "tkmk_memset");
                more |= box_fails(d, rest.ptr(), 0, rel_rows[d], 0, rel_cols[d]);
                for (size_t k = 0; k < n_drop; k++) check(tkmk_memcpy_d2d(rest.ptr() + drop[k], rho.ptr() + drop[k], sizeof(ScalarField)), "tkmk_memcpy_d2d");
            }
        }
        for (int d = 0; d < 2; d++) {
            if (!failed[d]) continue;
            Finding f;
            f.check = checks[d];
            if (systemic[d]) {
                f.section = "g2_points";
                f.what = std::string("sigma_2.") + coord[d] + " (g2_points[" + (d ? "8" : "9") + "]) is not the " + coord[d] + " of sigma_1." + coord[d] + ": e(sigma_1." + coord[d] +
                         ", H) != e(G, sigma_2." + coord[d] + "), so no record of xy_powers is at fault along " + (d ? "X" : "Y") + " and none was searched for";
            } else if (record != SIZE_MAX) {
                f.section = "xy_powers", f.index = (int64_t)record, f.row = (int64_t)(record / rs_y), f.col = (int64_t)(record % rs_y), f.more = more;
                f.what = "xy_powers[" + std::to_string(record) + "] (row " + std::to_string(record / rs_y) + ", col " + std::to_string(record % rs_y) +
                         ") is not [x^row y^col]G: it is in the first failing relation along Y and along X" +
                         (more ? "; with its relations set aside the table still fails: at least one more record is wrong" : "; every other relation of the table holds");
            } else {
                const size_t target = source[d] + (d ? rs_y : 1);
                f.section = "xy_powers", f.row = (int64_t)(target / rs_y), f.col = (int64_t)(target % rs_y), f.more = more;
                f.what = "xy_powers[" + std::to_string(target) + "] is not [" + coord[d] + "] xy_powers[" + std::to_string(source[d]) + "]: the first failing relation along " +
                         (d ? "X" : "Y") + "; which of the two records is wrong is not decided (" +
                         (found[1 - d] ? "the first failing relation of the other direction touches neither" : "the other direction has no failing relation") + ")" +
                         (more ? "; with this relation set aside the table still fails" : "");
            }
            rep.located.push_back(f);
        }
        rep.locate_s += since(t0);
    }
    if (!circuit) grid = DeviceVec<G1Affine>();
    rho = DeviceVec<ScalarField>();
    if (!rep.ratio_y) fail("xy_powers is not a table of powers along Y: sum rho P[a][b+1] != [y] sum rho P[a][b] for a random rho (a record is in the wrong place, or sigma_2.y is not [y]H)");
    if (!rep.ratio_x) fail("xy_powers is not a table of powers along X: sum rho P[a+1][b] != [x] sum rho P[a][b] for a random rho (a record is in the wrong place, or sigma_2.x is not [x]H)");
    rep.ok = rep.anchors == 1 && rep.ratio_y == 1 && rep.ratio_x == 1;
    if (circuit && rep.ok) {   // the table checks rest on xy_powers being right
        rep.circuit = audit_tables(crs, sp, lib_dir, grid, rep, locate) ? 1 : 0;
        if (!rep.circuit) rep.ok = false;
        grid = DeviceVec<G1Affine>();
    }
    return finish();
}

// <lib>/setupParams.json + <crs>/combined_sigma.{tkcrs, rkyv}, with `circuit` also <lib>/subcircuitInfo.json and <lib>/r1cs/; an unreadable
// file throws
inline bool audit_files(const std::string &lib_dir, const std::string &crs_dir, Report &rep, std::string *container = nullptr, bool circuit = false,
                        bool locate = false) {
    const SetupParams sp = SetupParams::read(lib_dir);
    validate_setup_shape(sp);
    const CrsPayload crs = load_combined_sigma(crs_dir, sp);
    if (container) *container = crs.container;
    return audit_payload(crs, sp, rep, circuit, lib_dir, locate);
}

// TKMK_PROVER_CHECK_CRS=1 (tkmk_prover_open): unset, empty or "0" = off; "2" = with the table checks against the circuit
inline bool requested_at_open() {
    const char *e = std::getenv("TKMK_PROVER_CHECK_CRS");
    return e && *e && std::strcmp(e, "0") != 0;
}
inline bool circuit_requested_at_open() {
    const char *e = std::getenv("TKMK_PROVER_CHECK_CRS");
    return e && std::strcmp(e, "2") == 0;
}

}  // namespace crs_audit
}  // namespace tkmk
