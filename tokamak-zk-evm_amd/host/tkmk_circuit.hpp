// tkmk_circuit.hpp — what a circuit looks like: the two static documents of a subcircuit library directory and its constraint files, with
// one reader and one shape check for the setup, `preprocess`, the CRS audit, the verifier, the resident prover (ProverContext::open_circuit)
// and through it the witness check (Prover::init still inlines its own).  Device-free (no call into libtkmk_hip.so), so the host-only verifier can include it.
//   SetupParams, validate_setup_shape                    <lib>/setupParams.json; setup_shape / validate_setup_shape (libs/src/utils/mod.rs:21-46);
//                                                        the shape of the CRS grid xy_powers that follows from it
//   SubcircuitInfo, SubcircuitLibrary                    <lib>/subcircuitInfo.json in file order (libs/src/iotools/mod.rs:458-469) and per
//                                                        entry <lib>/r1cs/subcircuit{id}.r1cs
//   R1csBinary / SubcircuitR1CS::from_r1cs_sparse_only   libs/src/iotools/mod.rs:505-760   (iden3 .r1cs v1, same validations)
//   flat_wire_owners                                     which library entry owns a flattened wire (the setup's write order)
// The per-proof documents (placementVariables.json, permutation.json, instance.json) are read by tkmk_inputs.hpp / tkmk_fastparse.hpp.
#pragma once
#include <array>
#include <fstream>
#include <iterator>

#include "tkmk_base.hpp"
#include "tkmk_fr.hpp"
#include "tkmk_json.hpp"

namespace tkmk {

struct SubcircuitInfo {
    size_t id;
    std::string name;
    size_t Nwires;
    std::array<size_t, 2> Out_idx, In_idx;   // [start, count]
    std::vector<size_t> flattenMap;
};
struct SetupParams {   // an aggregate: callers brace-initialise it in this order
    size_t l, l_user_out, l_user, l_free, l_D, m_D, n, s_D, s_max;

    // the interface wire count, and the grid of xy_powers: rs_x() rows of rs_y() records [x^h y^i]G (libs/src/group_structures/mod.rs:369-380).
    // Meaningful once validate_setup_shape has passed.
    size_t m_i() const { return l_D - l; }
    size_t rs_x() const { return std::max(2 * n, 2 * m_i()); }
    size_t rs_y() const { return 2 * s_max; }

    static SetupParams read(const std::string &lib_dir) {
        const json::Value jp = json::read_file(lib_dir + "/setupParams.json");
        return SetupParams{jp.at("l").as_size(),   jp.at("l_user_out").as_size(), jp.at("l_user").as_size(), jp.at("l_free").as_size(),
                           jp.at("l_D").as_size(), jp.at("m_D").as_size(),        jp.at("n").as_size(),      jp.at("s_D").as_size(),
                           jp.at("s_max").as_size()};
    }
};
// setup_shape / validate_setup_shape (libs/src/utils/mod.rs:21-46): what every user of the parameters relies on.  The checks of l_free,
// l_user and of a sharded prover's rank count stay with the callers that need them.
inline void validate_setup_shape(const SetupParams &sp) {
    if (sp.l_D < sp.l) throw Error("Invalid setup params: l_D must be >= l.");
    if (!is_pow2(sp.n)) throw Error("n is not a power of two.");
    if (!is_pow2(sp.s_max)) throw Error("s_max is not a power of two.");
    if (!is_pow2(sp.m_i())) throw Error("m_I is not a power of two.");
}

struct R1csError : Error {
    explicit R1csError(const std::string &m) : Error(m) {}
};

// r = BLS12-381 scalar modulus, little-endian u32 limbs (the prime in every committed .r1cs header)
inline ScalarField fr_from_le_bytes_mod_r(const uint8_t *p, size_t n) {
    // ScalarField::from_bytes_le on a field-size buffer: values below 2^256 reduced by repeated subtraction (at most twice)
    static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    ScalarField v{};
    std::memcpy(&v, p, n < 32 ? n : 32);
    for (size_t i = 32; i < n; i++)
        if (p[i]) throw R1csError("R1CS coefficient does not fit the scalar field");
    auto geq = [&]() {
        for (int i = 7; i >= 0; i--) {
            if (v.limbs[i] != R[i]) return v.limbs[i] > R[i];
        }
        return true;
    };
    while (geq()) {
        uint64_t br = 0;
        for (int i = 0; i < 8; i++) {
            uint64_t d = (uint64_t)v.limbs[i] - R[i] - br;
            v.limbs[i] = (uint32_t)d;
            br = (d >> 63) & 1;
        }
    }
    return v;
}

class R1csBinary {
  public:
    std::vector<uint8_t> data;
    size_t constraints_offset = 0, constraints_size = 0, field_size = 0;
    uint32_t n_wires = 0, n_constraints = 0;

    static R1csBinary read(const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw R1csError("cannot open " + path);
        return parse(std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()));
    }
    static R1csBinary parse(std::vector<uint8_t> bytes) {
        R1csBinary b;
        b.data = std::move(bytes);
        const auto &d = b.data;
        auto need = [&](size_t off, size_t n) {
            if (off + n > d.size()) throw R1csError("unexpected end of R1CS file");
        };
        auto u32 = [&](size_t off) {
            uint32_t v;
            std::memcpy(&v, d.data() + off, 4);
            return v;
        };
        auto u64 = [&](size_t off) {
            uint64_t v;
            std::memcpy(&v, d.data() + off, 8);
            return v;
        };
        need(0, 4);
        if (std::memcmp(d.data(), "r1cs", 4) != 0) throw R1csError("invalid R1CS magic");
        need(4, 8);
        uint32_t version = u32(4), sections = u32(8);
        if (version != 1) throw R1csError("unsupported R1CS version");
        size_t off = 12, hoff = 0, hsize = 0;
        bool have_h = false, have_c = false;
        for (uint32_t s = 0; s < sections; s++) {
            need(off, 12);
            uint32_t stype = u32(off);
            uint64_t ssize = u64(off + 4);
            off += 12;
            if (off + ssize > d.size()) throw R1csError("R1CS section extends past end of file");
            if (stype == 1) hoff = off, hsize = ssize, have_h = true;
            else if (stype == 2) b.constraints_offset = off, b.constraints_size = ssize, have_c = true;
            off += ssize;
        }
        if (!have_h) throw R1csError("missing R1CS header section");
        if (!have_c) throw R1csError("missing R1CS constraints section");
        size_t cur = hoff;
        need(cur, 4);
        b.field_size = u32(cur);
        cur += 4;
        if (b.field_size == 0 || b.field_size % 8) throw R1csError("invalid R1CS field size");
        need(cur, b.field_size + 28);
        cur += b.field_size;
        b.n_wires = u32(cur);
        cur += 16 + 8;   // nWires, nPubOut, nPubIn, nPrvIn, nLabels(u64)
        b.n_constraints = u32(cur);
        cur += 4;
        if (cur > hoff + hsize) throw R1csError("R1CS header extends past section end");
        return b;
    }
    std::vector<uint8_t> prime() const {   // the header's modulus, little-endian
        size_t off = 12;
        for (;;) {
            uint32_t stype;
            uint64_t ssize;
            std::memcpy(&stype, data.data() + off, 4);
            std::memcpy(&ssize, data.data() + off + 4, 8);
            off += 12;
            if (stype == 1) return std::vector<uint8_t>(data.begin() + off + 4, data.begin() + off + 4 + field_size);
            off += ssize;
        }
    }
};

// CSR rows of A, B, C
struct SubcircuitR1CS {
    uint32_t n_wires = 0, n_constraints = 0;
    std::vector<uint32_t> row_ptr[3], wire[3];
    std::vector<ScalarField> coeff[3];

    static SubcircuitR1CS from_r1cs_sparse_only(const R1csBinary &b, const SetupParams &sp, const SubcircuitInfo &info, size_t n_consts) {
        if (b.n_wires != info.Nwires) throw R1csError("R1CS nWires mismatch for subcircuit " + std::to_string(info.id));
        if (b.n_constraints != n_consts) throw R1csError("R1CS nConstraints mismatch for subcircuit " + std::to_string(info.id));
        if (sp.n < n_consts) throw R1csError("n is smaller than the actual number of constraints.");
        SubcircuitR1CS r;
        r.n_wires = b.n_wires;
        r.n_constraints = b.n_constraints;
        const auto &d = b.data;
        size_t off = b.constraints_offset, end = b.constraints_offset + b.constraints_size, fs = b.field_size;
        for (int m = 0; m < 3; m++) r.row_ptr[m].push_back(0);
        for (uint32_t row = 0; row < b.n_constraints; row++)
            for (int m = 0; m < 3; m++) {
                if (off + 4 > d.size()) throw R1csError("unexpected end of R1CS file");
                uint32_t cnt;
                std::memcpy(&cnt, d.data() + off, 4);
                off += 4;
                for (uint32_t k = 0; k < cnt; k++) {
                    if (off + 4 + fs > d.size()) throw R1csError("unexpected end of R1CS file");
                    uint32_t w;
                    std::memcpy(&w, d.data() + off, 4);
                    off += 4;
                    if (w >= b.n_wires) throw R1csError("R1CS wire index exceeds nWires");
                    r.wire[m].push_back(w);
                    r.coeff[m].push_back(fr_from_le_bytes_mod_r(d.data() + off, fs));
                    off += fs;
                }
                r.row_ptr[m].push_back((uint32_t)r.wire[m].size());
            }
        if (off != end) throw R1csError("R1CS constraints section has trailing bytes");
        return r;
    }
};

// The subcircuit library of a directory: <lib>/subcircuitInfo.json in file order, and per entry <lib>/r1cs/subcircuit{id}.r1cs.  A missing
// or malformed file throws.  read() is the whole library at once (the CRS audit); the trusted setup reads the constraint files one at a
// time through read_infos + read_r1cs.
struct SubcircuitLibrary {
    std::vector<SubcircuitInfo> infos;
    std::vector<size_t> n_consts;
    std::vector<SubcircuitR1CS> r1cs;   // by position in infos (filled by read() only)

    static SubcircuitLibrary read_infos(const std::string &lib_dir) {
        SubcircuitLibrary lib;
        const json::Value jinfo = json::read_file(lib_dir + "/subcircuitInfo.json");
        for (const json::Value &e : jinfo.items()) {
            SubcircuitInfo si;
            si.id = e.at("id").as_size();
            si.name = e.at("name").as_string();
            si.Nwires = e.at("Nwires").as_size();
            si.Out_idx = {e.at("Out_idx").items().at(0).as_size(), e.at("Out_idx").items().at(1).as_size()};
            si.In_idx = {e.at("In_idx").items().at(0).as_size(), e.at("In_idx").items().at(1).as_size()};
            for (const json::Value &g : e.at("flattenMap").items()) si.flattenMap.push_back(g.as_size());
            lib.infos.push_back(std::move(si));
            lib.n_consts.push_back(e.at("Nconsts").as_size());
        }
        return lib;
    }
    // entry s of the library (not subcircuit id s)
    static SubcircuitR1CS read_r1cs(const std::string &lib_dir, const SetupParams &sp, const SubcircuitInfo &info, size_t n_consts) {
        R1csBinary b = R1csBinary::read(lib_dir + "/r1cs/subcircuit" + std::to_string(info.id) + ".r1cs");
        return SubcircuitR1CS::from_r1cs_sparse_only(b, sp, info, n_consts);
    }
    static SubcircuitLibrary read(const std::string &lib_dir, const SetupParams &sp) {
        SubcircuitLibrary lib = read_infos(lib_dir);
        for (size_t k = 0; k < lib.infos.size(); k++) {
            const SubcircuitInfo &info = lib.infos[k];
            if (info.flattenMap.size() != info.Nwires) throw Error("subcircuitInfo.json: flattenMap length differs from Nwires for subcircuit " + std::to_string(info.id));
            lib.r1cs.push_back(read_r1cs(lib_dir, sp, info, lib.n_consts[k]));
        }
        return lib;
    }
};

// Which (entry s, local wire j) OWNS the flattened wire flattenMap[j]?  The setup's o_vec (evaled_qap_mixture, host/tkmk_setup.hpp) is
// written entry by entry, wire by wire, and only where o_j is non-zero, so a flattened index that several pairs map to keeps the value of
// the LAST pair, in that order, whose column of A, B or C holds an entry (a column with entries evaluates to zero at a random tau_x
// only with probability ~ n / r).  own[s][j] = 1 for that pair, 0 for every other: the CRS audit weights wires by it.
inline std::vector<std::vector<uint8_t>> flat_wire_owners(const std::vector<SubcircuitInfo> &infos, const std::vector<SubcircuitR1CS> &r1cs, size_t m_D) {
    if (infos.size() != r1cs.size()) throw Error("flat_wire_owners: one constraint system per library entry");
    std::vector<std::vector<uint8_t>> own(infos.size());
    std::vector<std::pair<uint32_t, uint32_t>> last(m_D, {UINT32_MAX, 0u});
    for (size_t s = 0; s < infos.size(); s++) {
        const SubcircuitR1CS &r = r1cs[s];
        if (infos[s].flattenMap.size() != r.n_wires) throw Error("subcircuitInfo.json: flattenMap length differs from Nwires for subcircuit " + std::to_string(infos[s].id));
        std::vector<uint8_t> used(r.n_wires, 0);
        for (int m = 0; m < 3; m++)
            for (size_t k = 0; k < r.wire[m].size(); k++)
                if (!fr_is_zero(r.coeff[m][k])) used[r.wire[m][k]] = 1;
        for (uint32_t j = 0; j < r.n_wires; j++) {
            if (!used[j]) continue;
            const size_t f = infos[s].flattenMap[j];
            if (f >= m_D) throw Error("subcircuitInfo.json: flattenMap entry outside the global wire range");
            last[f] = {(uint32_t)s, j};
        }
        own[s].assign(r.n_wires, 0);
    }
    for (const auto &p : last)
        if (p.first != UINT32_MAX) own[p.first][p.second] = 1;
    return own;
}

}  // namespace tkmk
