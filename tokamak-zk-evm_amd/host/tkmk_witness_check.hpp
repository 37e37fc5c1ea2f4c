// tkmk_witness_check.hpp — does a witness satisfy the circuit, and if not, where?  Three sections over what Prover::init has just put on
// the device (ProverContext::WitnessLoader, host/tkmk_service.hpp), each with its own verdict, all three always evaluated:
//   arithmetic   u . v = w in every cell of the n x s_max evaluation grids (tkmk_witness_check_r1cs): a placement whose variables do not
//                satisfy its subcircuit's R1CS is named with its first failing row
//   copy         b[row][col] = b[X][Y] for every entry of the EFFECTIVE permutation — the arrays after init's last-writer de-duplication
//                — and that map, extended by the identity on the cells no entry writes, is a bijection of the m_I x s_max cells (host, over
//                the bitmap of destinations)
//   public       every public wire of the four buffer placements equals the instance.json value at its flattenMap index (host: a few
//                hundred values that are already in the staging buffer)
// The reference has these diagnostics behind its `testing-mode` feature, as host loops over downloaded evaluations (prove/src/lib.rs:916-1017
// flag_b / flag_s0 / flag_s1 / flag_r, 1472-1518 "Placement indexed at {} does not satisfy R1CS").  What "wrong" means is what the verifier
// refuses: `ok` here equals tkmk_prover_verify's verdict on the proof the unguarded prover makes from the same documents
// (tests/test_gpu_witness_check.py).
//
// One code path for one rank and for G (run): rank r holds the columns c = r mod G of u, v, w, b — all of them when G = 1.  Each section
// writes what this rank found into a ShardBlock (counters, at most MAX_FINDINGS findings per section, an error text), and merge() makes the
// report from the blocks of all ranks: totals summed, findings in the order placement; entry; placement, wire, cut to MAX_FINDINGS.  With
// G = 1 the one block is merged as it stands and nothing is exchanged.  With G > 1 (collective: ProverContext::check_witness_sharded and
// the knob inside a sharded init) ONE tkmk_comm_all_gather_host carries the blocks, and every rank merges them into the same report.
//   arithmetic, public   local: a placement is a column, and only its owner staged its values.  An input error only one rank can see (the
//                public wires of placement 2 exist on its owner alone) travels in the block and is every rank's error, with one text.
//   copy         an entry ties cell (row, col) on rank col mod G to cell (X, Y) on rank Y mod G.  G = 1: tkmk_witness_check_copy over b.
//                G > 1: every rank knows the whole effective permutation, so every rank knows, without a message, the list S_s of entries
//                whose source lives on rank s (entry order).  Rank s packs those values of its b (tkmk_gather_rows_device), ONE
//                tkmk_comm_all_gather_dev of max_s |S_s| values per rank gives every rank all of them, and each rank compares its own
//                destination cells against its slots of the gathered buffer (tkmk_witness_check_copy_split).  A rank receives
//                G * max_s |S_s| * 32 bytes.  The destinations are distinct, so the sum of the |S_s| is at most the number of cells: evenly
//                spread sources make the payload at most one copy of b (m_I * s_max * 32 bytes, 128 MB at BASELINE.json configs[3]); the
//                padding to the longest list costs more when the sources crowd onto few ranks.
//
// Not covered: a sharded bin/witness-check / tkmk_witness_check_files (there is no sharded context without a reference string), BN254,
// WHICH variable of a failing row is wrong, and an all-to-all in place of the all-gather (a rank needs only the sources of its own
// entries; the all-gather is the collective that exists on both transports).
#pragma once
#include <algorithm>
#include <cstring>

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

// What the three sections read on rank shard.rank of shard.world.  Device pointers are borrowed and are this rank's columns: u, v, w
// (n x lc) and b (m_I x lc), element (row, local column k) at row * lc + k; local column k is global column rank + k G.  One rank: lc =
// s_max, every placement and every entry is this rank's, the local destinations are perm's own.
struct Inputs {
    const SetupParams *sp = nullptr;
    const std::vector<SubcircuitInfo> *infos = nullptr;
    const WitnessLayout *layout = nullptr;      // kind and first staged value of every placement
    const ScalarField *staged = nullptr;        // the parsed witness on the host (the pinned staging buffer)
    const ScalarField *u = nullptr, *v = nullptr, *w = nullptr, *b = nullptr;
    const EffectivePermutation *perm = nullptr;           // the replicated whole, global indices
    const std::vector<uint32_t> *local_entry = nullptr;   // this rank's entries: index into perm's arrays, ascending; null: all of them
    const std::vector<uint32_t> *local_dst = nullptr;     // ... and their destinations row * lc + col / G
    const uint32_t *d_dst = nullptr, *d_x = nullptr, *d_y = nullptr;   // local_dst and its sources X, Y on the device (null when empty; X, Y are read by one rank only)
    const std::vector<ScalarField> *a_pub_user = nullptr, *a_pub_block = nullptr, *a_pub_function = nullptr;
    Shard shard;
    const ShardLink *link = nullptr;            // the communicator of shard.world > 1; not used by one rank
    size_t lc = 0, placements = 0;              // this rank's columns of s_max, and its placements (the first `placements` columns)
};

// the block a rank contributes to the merge: plain data of one size on every rank
struct ShardBlock {
    struct Arithmetic {
        uint64_t placement;
        uint32_t first_row, bad_rows;
        ScalarField u, v, w;
    };
    struct Copy {
        uint64_t entry;
        ScalarField value, source;
    };
    struct Public {
        uint64_t index, placement, wire;
        ScalarField value, instance;
    };
    uint64_t bad_cells, bad_placements, n_arithmetic;
    uint64_t bad_entries, n_copy;
    uint64_t wires, bad_public, n_public;
    Arithmetic arithmetic[MAX_FINDINGS];
    Copy copy[MAX_FINDINGS];
    Public pub[MAX_FINDINGS];
    uint32_t failed, failed_placement;   // an input error this rank alone could see, in that placement: `error` holds its text
    char error[248];
};
static_assert(std::is_trivially_copyable<ShardBlock>::value, "ShardBlock travels as bytes");

// this rank's columns of the arithmetic section: local column k is placement rank + k G
inline void arithmetic_section(const Inputs &in, ShardBlock &blk) {
    const size_t n = in.sp->n, PL = in.placements, G = in.shard.world, rank = in.shard.rank;
    if (!PL) return;
    DeviceVec<uint32_t> d_cnt(PL), d_first(PL);
    check(tkmk_witness_check_r1cs(in.u, in.v, in.w, (uint32_t)n, (uint32_t)PL, (uint32_t)in.lc, d_cnt.ptr(), d_first.ptr(), &blk.bad_cells, nullptr), "tkmk_witness_check_r1cs");
    if (!blk.bad_cells) return;
    std::vector<uint32_t> cnt(PL), first(PL);
    d_cnt.copy_to_host(cnt.data(), PL), d_first.copy_to_host(first.data(), PL);
    for (size_t k = 0; k < PL; k++) {
        if (!cnt[k]) continue;
        blk.bad_placements++;
        if (blk.n_arithmetic >= MAX_FINDINGS) continue;
        ShardBlock::Arithmetic &f = blk.arithmetic[blk.n_arithmetic++];
        f.placement = rank + k * G, f.first_row = first[k], f.bad_rows = cnt[k];
        const size_t at = (size_t)first[k] * in.lc + k;
        check(tkmk_memcpy_d2h(&f.u, in.u + at, sizeof(ScalarField)), "memcpy_d2h");
        check(tkmk_memcpy_d2h(&f.v, in.v + at, sizeof(ScalarField)), "memcpy_d2h");
        check(tkmk_memcpy_d2h(&f.w, in.w + at, sizeof(ScalarField)), "memcpy_d2h");
    }
}

// The first MAX_FINDINGS failing ones of this rank's n entries (the local lists ascend in the global entry index).  compare(from, &bad,
// &first) counts the failing entries of [from, n) and names the first of them relative to `from`, so the next search starts behind it;
// source_of(k) is where entry k's source value lies on the device.
template <class Compare, class SourceOf>
inline void copy_walk(const Inputs &in, uint64_t n, ShardBlock &blk, Compare compare, SourceOf source_of) {
    uint64_t from = 0;
    while (from < n) {
        uint64_t bad = 0, first = UINT64_MAX;
        compare(from, &bad, &first);
        if (from == 0) blk.bad_entries = bad;
        if (!bad || blk.n_copy >= MAX_FINDINGS) break;
        const uint64_t k = from + first;
        ShardBlock::Copy &f = blk.copy[blk.n_copy++];
        f.entry = in.local_entry ? (*in.local_entry)[k] : k;
        check(tkmk_memcpy_d2h(&f.value, in.b + (*in.local_dst)[k], sizeof(ScalarField)), "memcpy_d2h");
        check(tkmk_memcpy_d2h(&f.source, source_of(k), sizeof(ScalarField)), "memcpy_d2h");
        from = k + 1;
    }
}

// the values of the copy section.  One rank: the entries against b itself.  G ranks: the one device all-gather, then this rank's entries
// against the gathered sources
inline void copy_section(const Inputs &in, ShardBlock &blk) {
    const size_t s_max = in.sp->s_max, m_i = in.sp->m_i(), G = in.shard.world, rank = in.shard.rank, lc = in.lc;
    const EffectivePermutation &ep = *in.perm;
    const size_t E = ep.dst.size();
    if (G == 1) {
        copy_walk(
            in, E, blk,
            [&](uint64_t from, uint64_t *bad, uint64_t *first) {
                check(tkmk_witness_check_copy(in.b, (uint32_t)m_i, (uint32_t)s_max, (uint32_t)s_max, in.d_dst + from, in.d_x + from, in.d_y + from, E - from, bad, first, nullptr),
                      "tkmk_witness_check_copy");
            },
            [&](uint64_t e) { return in.b + (size_t)ep.x[e] * s_max + ep.y[e]; });
        return;
    }
    // S_s, from the replicated arrays alone: entry e is number pos[e] of the entries whose source column Y lives on rank Y mod G
    std::vector<uint32_t> pos(E), count(G, 0), mine;
    for (size_t e = 0; e < E; e++) {
        const uint32_t owner = ep.y[e] % (uint32_t)G;
        pos[e] = count[owner]++;
        if (owner == rank) mine.push_back(ep.x[e] * (uint32_t)lc + ep.y[e] / (uint32_t)G);   // the source cell in this rank's b
    }
    const size_t pad = *std::max_element(count.begin(), count.end());
    if (!pad) return;   // no entry anywhere: every rank returns here
    if (G * pad >= (1ull << 32)) throw Error("witness check: more gathered source values than a 32-bit slot can name");
    DeviceVec<ScalarField> send(pad), sources(G * pad);
    check(tkmk_memset(send.ptr(), 0, pad * sizeof(ScalarField)), "memset");
    if (!mine.empty()) {
        DeviceVec<uint32_t> d_mine = DeviceVec<uint32_t>::from_host(mine);
        check(tkmk_gather_rows_device(in.b, sizeof(ScalarField), d_mine.ptr(), mine.size(), send.ptr(), nullptr), "tkmk_gather_rows_device");
        check(tkmk_device_synchronize(), "synchronize");   // d_mine goes here
    }
    check(in.link->all_gather_dev(in.link->comm, send.ptr(), pad * sizeof(ScalarField), sources.ptr()), "tkmk_comm_all_gather_dev");
    const std::vector<uint32_t> &entry = *in.local_entry;
    const size_t n = entry.size();
    if (!n) return;
    std::vector<uint32_t> slot(n);
    for (size_t k = 0; k < n; k++) slot[k] = (ep.y[entry[k]] % (uint32_t)G) * (uint32_t)pad + pos[entry[k]];
    DeviceVec<uint32_t> d_slot = DeviceVec<uint32_t>::from_host(slot);
    copy_walk(
        in, n, blk,
        [&](uint64_t from, uint64_t *bad, uint64_t *first) {
            check(tkmk_witness_check_copy_split(in.b, m_i * lc, in.d_dst + from, sources.ptr(), G * pad, d_slot.ptr() + from, n - from, bad, first, nullptr),
                  "tkmk_witness_check_copy_split");
        },
        [&](uint64_t k) { return sources.ptr() + slot[k]; });
}

// the public wires of the four buffer placements (encode_O_pub_free / encode_O_pub_fix, libs/src/group_structures/mod.rs:145-229: the outputs
// of bufferPubOut, the inputs of bufferPubIn / bufferBlockIn / bufferEVMIn) against a_pub_user ++ a_pub_block ++ a_pub_function
// — those of placement q, which the rank that staged its values checks
inline void check_public(const Inputs &in, ShardBlock &blk, size_t q) {
    const SetupParams &sp = *in.sp;
    if (q >= in.layout->id.size()) return;
    const SubcircuitInfo &info = in.infos->at(in.layout->id[q]);
    const std::array<size_t, 2> *rng = nullptr;
    if (info.name == "bufferPubOut") rng = &info.Out_idx;
    else if (info.name == "bufferPubIn" || info.name == "bufferBlockIn" || info.name == "bufferEVMIn") rng = &info.In_idx;
    if (!rng) return;
    for (size_t j = (*rng)[0]; j < (*rng)[0] + (*rng)[1]; j++) {
        if (j >= info.Nwires) throw Error("subcircuitInfo.json: public wire range outside the subcircuit");
        const size_t g = info.flattenMap[j];
        if (g >= sp.l) throw Error("subcircuitInfo.json: public wire mapped outside [0, l)");
        const std::vector<ScalarField> &src = g < sp.l_user ? *in.a_pub_user : g < sp.l_free ? *in.a_pub_block : *in.a_pub_function;
        const size_t at = g < sp.l_user ? g : g < sp.l_free ? g - sp.l_user : g - sp.l_free;
        if (at >= src.size()) throw Error("instance.json: no value for public wire " + std::to_string(g));
        const ScalarField &val = in.staged[in.layout->off[q] + j];
        blk.wires++;
        if (fr_eq(val, src[at])) continue;
        blk.bad_public++;
        if (blk.n_public < MAX_FINDINGS) blk.pub[blk.n_public++] = ShardBlock::Public{g, q, j, val, src[at]};
    }
}

// the verdict and `reason` from the three sections' findings
inline bool conclude(Report &rep) {
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

// this rank's share of the public section: placement q < 4 is checked by rank q mod G, the only one that staged its values.  G ranks: an
// input error is carried in the block (merge makes it every rank's); one rank: it leaves as it is
inline void public_section(const Inputs &in, ShardBlock &blk) {
    const size_t G = in.shard.world;
    for (size_t q = in.shard.rank; q < 4 && !blk.failed; q += G) {
        try {
            check_public(in, blk, q);
        } catch (const Error &e) {
            if (G == 1 || e.code != TKMK_ERR_INVALID_ARGUMENT) throw;
            blk.failed = 1, blk.failed_placement = (uint32_t)q;
            snprintf(blk.error, sizeof blk.error, "%s", e.what());
        }
    }
}

// The report from every rank's block (rank order; one block when there is one rank): host work over replicated data alone, so the same
// on every rank.  A block's input error is thrown — the text of the lowest failing placement, as a walk over all placements would meet it.
inline bool merge(const Inputs &in, const std::vector<ShardBlock> &all, Report &rep) {
    const size_t s_max = in.sp->s_max;
    const EffectivePermutation &ep = *in.perm;
    const ShardBlock *failed = nullptr;
    for (const ShardBlock &b : all)
        if (b.failed && (!failed || b.failed_placement < failed->failed_placement)) failed = &b;
    if (failed) throw Error(std::string(failed->error, strnlen(failed->error, sizeof failed->error)));
    rep.arithmetic.placements = in.layout->id.size();
    rep.copy.entries = ep.dst.size();
    uint32_t twice = 0;
    rep.copy.bijection = is_bijection(ep, s_max, &twice);
    rep.copy.twice_row = twice / (uint32_t)s_max, rep.copy.twice_col = twice % (uint32_t)s_max;
    std::vector<ShardBlock::Arithmetic> fa;
    std::vector<ShardBlock::Copy> fc;
    std::vector<ShardBlock::Public> fp;
    for (const ShardBlock &b : all) {
        rep.arithmetic.bad_cells += b.bad_cells, rep.arithmetic.bad_placements += b.bad_placements;
        rep.copy.bad_entries += b.bad_entries;
        rep.pub.wires += b.wires, rep.pub.bad += b.bad_public;
        if (b.n_arithmetic > MAX_FINDINGS || b.n_copy > MAX_FINDINGS || b.n_public > MAX_FINDINGS) throw Error(TKMK_ERR_UNKNOWN, "witness check: a rank's block is malformed");
        fa.insert(fa.end(), b.arithmetic, b.arithmetic + b.n_arithmetic);
        fc.insert(fc.end(), b.copy, b.copy + b.n_copy);
        fp.insert(fp.end(), b.pub, b.pub + b.n_public);
    }
    std::sort(fa.begin(), fa.end(), [](const ShardBlock::Arithmetic &a, const ShardBlock::Arithmetic &b) { return a.placement < b.placement; });
    std::sort(fc.begin(), fc.end(), [](const ShardBlock::Copy &a, const ShardBlock::Copy &b) { return a.entry < b.entry; });
    std::sort(fp.begin(), fp.end(), [](const ShardBlock::Public &a, const ShardBlock::Public &b) { return a.placement != b.placement ? a.placement < b.placement : a.wire < b.wire; });
    for (size_t k = 0; k < fa.size() && k < MAX_FINDINGS; k++) {
        const SubcircuitInfo &info = in.infos->at(in.layout->id.at(fa[k].placement));
        rep.arithmetic.first.push_back(ArithmeticFinding{(size_t)fa[k].placement, info.id, info.name, fa[k].first_row, fa[k].bad_rows, fa[k].u, fa[k].v, fa[k].w});
    }
    for (size_t k = 0; k < fc.size() && k < MAX_FINDINGS; k++) {
        const uint64_t e = fc[k].entry;
        rep.copy.first.push_back(CopyFinding{e, ep.dst.at(e) / (uint32_t)s_max, ep.dst.at(e) % (uint32_t)s_max, ep.x.at(e), ep.y.at(e), fc[k].value, fc[k].source});
    }
    for (size_t k = 0; k < fp.size() && k < MAX_FINDINGS; k++)
        rep.pub.first.push_back(PublicFinding{(size_t)fp[k].index, (size_t)fp[k].placement, (size_t)fp[k].wire, fp[k].value, fp[k].instance});
    rep.arithmetic.ok = rep.arithmetic.bad_cells == 0;
    rep.copy.ok = rep.copy.bijection && rep.copy.bad_entries == 0;
    rep.pub.ok = rep.pub.bad == 0;
    return conclude(rep);
}

// The three sections on rank in.shard.rank of G = in.shard.world, then the merge.  G > 1 is collective: every rank calls it, every rank
// gets the same report and verdict.  Exchanges: one tkmk_comm_all_gather_dev (none when the permutation is empty) and one
// tkmk_comm_all_gather_host; none at all with G = 1, communicator or not.  A device or transport failure leaves as an exception with the
// peers possibly waiting: the caller aborts the communicator (ProverContext does).
inline bool run(const Inputs &in, Report &rep) {
    ShardBlock blk;
    std::memset(&blk, 0, sizeof blk);
    arithmetic_section(in, blk);
    copy_section(in, blk);
    public_section(in, blk);
    std::vector<ShardBlock> all(in.shard.world, blk);
    if (in.shard.world > 1) check(in.link->all_gather_host(in.link->comm, &blk, sizeof blk, all.data()), "tkmk_comm_all_gather_host");
    return merge(in, all, rep);
}
}  // namespace witness_check
}  // namespace tkmk
