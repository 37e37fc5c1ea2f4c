// tkmk_witness_check.hpp — does a witness satisfy the circuit, and if not, where?  Three sections over what Prover::init has just put on
// the device (ProverContext::WitnessLoader, host/tkmk_service.hpp), each with its own verdict, all three always evaluated:
//   arithmetic   u . v = w in every cell of the n x s_max evaluation grids (tkmk_witness_check_r1cs): a placement whose variables do not
//                satisfy its subcircuit's R1CS is named with its first failing row
//   copy         b[row][col] = b[X][Y] for every entry of the EFFECTIVE permutation — the arrays after init's last-writer de-duplication
//                (tkmk_witness_check_copy) — and that map, extended by the identity on the cells no entry writes, is a bijection of
//                the m_I x s_max cells (host, over the bitmap of destinations)
//   public       every public wire of the four buffer placements equals the instance.json value at its flattenMap index (host: a few
//                hundred values that are already in the staging buffer)
// The reference has these diagnostics behind its `testing-mode` feature, as host loops over downloaded evaluations (prove/src/lib.rs:916-1017
// flag_b / flag_s0 / flag_s1 / flag_r, 1472-1518 "Placement indexed at {} does not satisfy R1CS").  What "wrong" means is what the verifier
// refuses: `ok` here equals tkmk_prover_verify's verdict on the proof the unguarded prover makes from the same documents
// (tests/test_gpu_witness_check.py).  Not covered: sharded contexts (the copy section crosses columns), BN254, and WHICH variable of a
// failing row is wrong.
#pragma once
#include "tkmk_circuit.hpp"
#include "tkmk_fastparse.hpp"
#include "tkmk_host.hpp"

namespace tkmk {
namespace witness_check {

constexpr size_t MAX_FINDINGS = 8;   // per section

// TKMK_PROVER_CHECK_WITNESS=1: tkmk_prover_prove[_ex] and bin/prove run the three sections inside init, before the binding commitments.
// Unset or 0: nothing is launched and nothing is downloaded.  Read per call (a resident service may switch it between proofs).
inline bool requested_at_prove() {
    const char *e = getenv("TKMK_PROVER_CHECK_WITNESS");
    return e && atoi(e) != 0;
}

inline std::string fr_hex(const ScalarField &v) {   // 0x + 64 hex digits, most significant first
    static const char *digits = "0123456789abcdef";
    std::string s = "0x";
    for (int i = 7; i >= 0; i--)
        for (int sh = 28; sh >= 0; sh -= 4) s += digits[(v.limbs[i] >> sh) & 15];
    return s;
}

// Permutation::to_poly's redirects (libs/src/iotools/mod.rs:438-448) as init issues them: distinct destinations dst = row * s_max + col —
// the reference's serial loop lets the LAST entry of a cell win — with their sources.  `written` is the bitmap of destinations.
struct EffectivePermutation {
    std::vector<uint32_t> dst, x, y;
    std::vector<uint64_t> written;
};
inline EffectivePermutation effective_permutation(const PermutationColumns &perm, size_t m_i, size_t s_max) {
    EffectivePermutation ep;
    const size_t cells = m_i * s_max;
    std::vector<uint64_t> &bitmap = ep.written;
    bitmap.assign((cells + 63) / 64, 0);
    bool dup = false;
    ep.dst.reserve(perm.size());
    for (size_t e = 0; e < perm.size(); e++) {
        if (perm.row[e] >= m_i || perm.col[e] >= s_max || perm.X[e] >= m_i || perm.Y[e] >= s_max) throw Error("permutation entry out of range");
        uint32_t d = perm.row[e] * (uint32_t)s_max + perm.col[e];
        if (bitmap[d >> 6] >> (d & 63) & 1) dup = true;
        bitmap[d >> 6] |= 1ull << (d & 63);
        ep.dst.push_back(d);
    }
    ep.x = perm.X, ep.y = perm.Y;
    if (dup) {   // keep the last writer of every cell
        std::fill(bitmap.begin(), bitmap.end(), 0);
        std::vector<uint32_t> d2, x2, y2;
        for (size_t e = perm.size(); e-- > 0;) {
            uint32_t d = ep.dst[e];
            if (bitmap[d >> 6] >> (d & 63) & 1) continue;
            bitmap[d >> 6] |= 1ull << (d & 63);
            d2.push_back(d), x2.push_back(ep.x[e]), y2.push_back(ep.y[e]);
        }
        ep.dst.swap(d2), ep.x.swap(x2), ep.y.swap(y2);
    }
    return ep;
}
// Is cell -> (X, Y) on the written cells, the identity elsewhere, a bijection of the cells?  The destinations are distinct, so it is one
// exactly when the sources are distinct and every source is itself a written cell (an unwritten cell already maps to itself).  Otherwise
// *twice names a cell that two cells map to.
inline bool is_bijection(const EffectivePermutation &ep, size_t s_max, uint32_t *twice) {
    std::vector<uint64_t> seen(ep.written.size(), 0);
    for (size_t e = 0; e < ep.dst.size(); e++) {
        const uint32_t s = ep.x[e] * (uint32_t)s_max + ep.y[e];
        const bool unwritten = !(ep.written[s >> 6] >> (s & 63) & 1), again = seen[s >> 6] >> (s & 63) & 1;
        if (unwritten || again) {
            *twice = s;
            return false;
        }
        seen[s >> 6] |= 1ull << (s & 63);
    }
    return true;
}

struct ArithmeticFinding {
    size_t placement, subcircuit_id;
    std::string name;
    uint32_t first_row, bad_rows;
    ScalarField u, v, w;   // at (first_row, placement)
};
struct CopyFinding {
    uint64_t entry;   // index into the effective arrays
    uint32_t row, col, X, Y;
    ScalarField value, source;
};
struct PublicFinding {
    size_t index, placement, wire;   // index = flattenMap[wire] into a_pub_user ++ a_pub_block ++ a_pub_function
    ScalarField value, instance;
};
struct Report {
    bool ok = false;
    std::string reason;   // the first finding of the first failing section
    struct {
        bool ok = false;
        size_t placements = 0, bad_placements = 0;
        uint64_t bad_cells = 0;
        std::vector<ArithmeticFinding> first;
    } arithmetic;
    struct {
        bool ok = false, bijection = false;
        uint64_t entries = 0, bad_entries = 0;
        uint32_t twice_row = 0, twice_col = 0;   // when !bijection
        std::vector<CopyFinding> first;
    } copy;
    struct {
        bool ok = false;
        size_t wires = 0, bad = 0;
        std::vector<PublicFinding> first;
    } pub;
    double parse_s = 0, upload_s = 0, build_s = 0, check_s = 0, total_s = 0;

    static std::string quoted(const std::string &s) {
        std::string o = "\"";
        for (char c : s) {
            if (c == '"' || c == '\\') o += '\\';
            if ((unsigned char)c < 0x20) c = ' ';
            o += c;
        }
        return o + "\"";
    }
    std::string to_json() const {
        auto b = [](bool v) { return v ? "true" : "false"; };
        auto n = [](uint64_t v) { return std::to_string(v); };
        std::string d = std::string("{\"ok\": ") + b(ok) + ", \"reason\": " + quoted(reason);
        d += std::string(", \"arithmetic\": {\"ok\": ") + b(arithmetic.ok) + ", \"placements\": " + n(arithmetic.placements) + ", \"bad_placements\": " +
             n(arithmetic.bad_placements) + ", \"bad_cells\": " + n(arithmetic.bad_cells) + ", \"first\": [";
        for (size_t k = 0; k < arithmetic.first.size(); k++) {
            const ArithmeticFinding &f = arithmetic.first[k];
            d += std::string(k ? ", " : "") + "{\"placement\": " + n(f.placement) + ", \"subcircuitId\": " + n(f.subcircuit_id) + ", \"name\": " + quoted(f.name) +
                 ", \"first_row\": " + n(f.first_row) + ", \"bad_rows\": " + n(f.bad_rows) + ", \"u\": \"" + fr_hex(f.u) + "\", \"v\": \"" + fr_hex(f.v) + "\", \"w\": \"" +
                 fr_hex(f.w) + "\"}";
        }
        d += std::string("]}, \"copy\": {\"ok\": ") + b(copy.ok) + ", \"entries\": " + n(copy.entries) + ", \"bijection\": " + b(copy.bijection);
        if (!copy.bijection) d += ", \"hit_twice\": {\"row\": " + n(copy.twice_row) + ", \"col\": " + n(copy.twice_col) + "}";
        d += ", \"bad_entries\": " + n(copy.bad_entries) + ", \"first\": [";
        for (size_t k = 0; k < copy.first.size(); k++) {
            const CopyFinding &f = copy.first[k];
            d += std::string(k ? ", " : "") + "{\"entry\": " + n(f.entry) + ", \"row\": " + n(f.row) + ", \"col\": " + n(f.col) + ", \"X\": " + n(f.X) + ", \"Y\": " + n(f.Y) +
                 ", \"value\": \"" + fr_hex(f.value) + "\", \"source\": \"" + fr_hex(f.source) + "\"}";
        }
        d += std::string("]}, \"public\": {\"ok\": ") + b(pub.ok) + ", \"wires\": " + n(pub.wires) + ", \"bad\": " + n(pub.bad) + ", \"first\": [";
        for (size_t k = 0; k < pub.first.size(); k++) {
            const PublicFinding &f = pub.first[k];
            d += std::string(k ? ", " : "") + "{\"index\": " + n(f.index) + ", \"placement\": " + n(f.placement) + ", \"wire\": " + n(f.wire) + ", \"value\": \"" +
                 fr_hex(f.value) + "\", \"instance\": \"" + fr_hex(f.instance) + "\"}";
        }
        char t[256];
        snprintf(t, sizeof t, "]}, \"seconds\": {\"parse\": %.6f, \"upload\": %.6f, \"build\": %.6f, \"check\": %.6f, \"total\": %.6f}}", parse_s, upload_s, build_s, check_s,
                 total_s);
        return d + t;
    }
};

// What the three sections read.  Device pointers are borrowed; everything is the unsharded form (element (row, col) at row * s_max + col).
struct Inputs {
    const SetupParams *sp = nullptr;
    const std::vector<SubcircuitInfo> *infos = nullptr;
    const WitnessLayout *layout = nullptr;      // kind and first staged value of every placement
    const ScalarField *staged = nullptr;        // the parsed witness on the host (the pinned staging buffer)
    const ScalarField *u = nullptr, *v = nullptr, *w = nullptr, *b = nullptr;             // n x s_max (u, v, w) and m_I x s_max (b) on the device
    const EffectivePermutation *perm = nullptr;
    const uint32_t *d_dst = nullptr, *d_x = nullptr, *d_y = nullptr;                      // perm's three arrays on the device (null when it is empty)
    const std::vector<ScalarField> *a_pub_user = nullptr, *a_pub_block = nullptr, *a_pub_function = nullptr;
};

inline void check_arithmetic(const Inputs &in, Report &rep) {
    const size_t s_max = in.sp->s_max, n = in.sp->n, P = in.layout->id.size();
    auto &sec = rep.arithmetic;
    sec.placements = P;
    if (P) {
        DeviceVec<uint32_t> d_cnt(P), d_first(P);
        check(tkmk_witness_check_r1cs(in.u, in.v, in.w, (uint32_t)n, (uint32_t)P, (uint32_t)s_max, d_cnt.ptr(), d_first.ptr(), &sec.bad_cells, nullptr), "tkmk_witness_check_r1cs");
        if (sec.bad_cells) {
            std::vector<uint32_t> cnt(P), first(P);
            d_cnt.copy_to_host(cnt.data(), P), d_first.copy_to_host(first.data(), P);
            for (size_t q = 0; q < P; q++) {
                if (!cnt[q]) continue;
                sec.bad_placements++;
                if (sec.first.size() >= MAX_FINDINGS) continue;
                const SubcircuitInfo &info = in.infos->at(in.layout->id[q]);
                ArithmeticFinding f{q, info.id, info.name, first[q], cnt[q], {}, {}, {}};
                const size_t at = (size_t)first[q] * s_max + q;
                check(tkmk_memcpy_d2h(&f.u, in.u + at, sizeof(ScalarField)), "memcpy_d2h");
                check(tkmk_memcpy_d2h(&f.v, in.v + at, sizeof(ScalarField)), "memcpy_d2h");
                check(tkmk_memcpy_d2h(&f.w, in.w + at, sizeof(ScalarField)), "memcpy_d2h");
                sec.first.push_back(std::move(f));
            }
        }
    }
    sec.ok = sec.bad_cells == 0;
}

inline void check_copy(const Inputs &in, Report &rep) {
    const size_t s_max = in.sp->s_max, m_i = in.sp->m_i();
    const EffectivePermutation &ep = *in.perm;
    auto &sec = rep.copy;
    sec.entries = ep.dst.size();
    uint32_t twice = 0;
    sec.bijection = is_bijection(ep, s_max, &twice);
    sec.twice_row = twice / (uint32_t)s_max, sec.twice_col = twice % (uint32_t)s_max;
    // the first MAX_FINDINGS failing entries: the kernel names the first one of a range, so the next search starts behind it
    uint64_t from = 0;
    while (from < sec.entries) {
        uint64_t bad = 0, first = UINT64_MAX;
        check(tkmk_witness_check_copy(in.b, (uint32_t)m_i, (uint32_t)s_max, (uint32_t)s_max, in.d_dst + from, in.d_x + from, in.d_y + from, sec.entries - from, &bad, &first, nullptr),
              "tkmk_witness_check_copy");
        if (from == 0) sec.bad_entries = bad;
        if (!bad || sec.first.size() >= MAX_FINDINGS) break;
        const uint64_t e = from + first;
        CopyFinding f{e, ep.dst[e] / (uint32_t)s_max, ep.dst[e] % (uint32_t)s_max, ep.x[e], ep.y[e], {}, {}};
        check(tkmk_memcpy_d2h(&f.value, in.b + ep.dst[e], sizeof(ScalarField)), "memcpy_d2h");
        check(tkmk_memcpy_d2h(&f.source, in.b + (size_t)f.X * s_max + f.Y, sizeof(ScalarField)), "memcpy_d2h");
        sec.first.push_back(f);
        from = e + 1;
    }
    sec.ok = sec.bijection && sec.bad_entries == 0;
}

// the public wires of the four buffer placements (encode_O_pub_free / encode_O_pub_fix, libs/src/group_structures/mod.rs:145-229: the outputs
// of bufferPubOut, the inputs of bufferPubIn / bufferBlockIn / bufferEVMIn) against a_pub_user ++ a_pub_block ++ a_pub_function
inline void check_public(const Inputs &in, Report &rep) {
    const SetupParams &sp = *in.sp;
    auto &sec = rep.pub;
    const size_t P = std::min<size_t>(4, in.layout->id.size());
    for (size_t q = 0; q < P; q++) {
        const SubcircuitInfo &info = in.infos->at(in.layout->id[q]);
        const std::array<size_t, 2> *rng = nullptr;
        if (info.name == "bufferPubOut") rng = &info.Out_idx;
        else if (info.name == "bufferPubIn" || info.name == "bufferBlockIn" || info.name == "bufferEVMIn") rng = &info.In_idx;
        if (!rng) continue;
        for (size_t j = (*rng)[0]; j < (*rng)[0] + (*rng)[1]; j++) {
            if (j >= info.Nwires) throw Error("subcircuitInfo.json: public wire range outside the subcircuit");
            const size_t g = info.flattenMap[j];
            if (g >= sp.l) throw Error("subcircuitInfo.json: public wire mapped outside [0, l)");
            const std::vector<ScalarField> &src = g < sp.l_user ? *in.a_pub_user : g < sp.l_free ? *in.a_pub_block : *in.a_pub_function;
            const size_t at = g < sp.l_user ? g : g < sp.l_free ? g - sp.l_user : g - sp.l_free;
            if (at >= src.size()) throw Error("instance.json: no value for public wire " + std::to_string(g));
            const ScalarField &val = in.staged[in.layout->off[q] + j];
            sec.wires++;
            if (fr_eq(val, src[at])) continue;
            sec.bad++;
            if (sec.first.size() < MAX_FINDINGS) sec.first.push_back(PublicFinding{g, q, j, val, src[at]});
        }
    }
    sec.ok = sec.bad == 0;
}

inline bool run(const Inputs &in, Report &rep) {
    check_arithmetic(in, rep);
    check_copy(in, rep);
    check_public(in, rep);
    rep.ok = rep.arithmetic.ok && rep.copy.ok && rep.pub.ok;
    rep.reason.clear();
    if (!rep.arithmetic.ok) {
        const ArithmeticFinding &f = rep.arithmetic.first.front();
        rep.reason = "arithmetic: placement " + std::to_string(f.placement) + " (subcircuit " + std::to_string(f.subcircuit_id) + ", " + f.name +
                     ") does not satisfy its R1CS: " + std::to_string(f.bad_rows) + " failing row(s), the first is row " + std::to_string(f.first_row);
    } else if (!rep.copy.ok) {
        if (!rep.copy.bijection)
            rep.reason = "copy: the permutation is not a bijection: cell (row " + std::to_string(rep.copy.twice_row) + ", col " + std::to_string(rep.copy.twice_col) +
                         ") is the image of two cells";
        else {
            const CopyFinding &f = rep.copy.first.front();
            rep.reason = "copy: entry " + std::to_string(f.entry) + " (row " + std::to_string(f.row) + ", col " + std::to_string(f.col) + ") differs from its source (X " +
                         std::to_string(f.X) + ", Y " + std::to_string(f.Y) + "): " + std::to_string(rep.copy.bad_entries) + " failing entries";
        }
    } else if (!rep.pub.ok) {
        const PublicFinding &f = rep.pub.first.front();
        rep.reason = "public: wire " + std::to_string(f.wire) + " of placement " + std::to_string(f.placement) + " differs from instance.json at public index " +
                     std::to_string(f.index) + ": " + std::to_string(rep.pub.bad) + " mismatch(es)";
    }
    return rep.ok;
}

}  // namespace witness_check
}  // namespace tkmk
