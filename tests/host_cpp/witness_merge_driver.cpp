// test driver for witness_check::merge of host/tkmk_witness_check.hpp (CPU only: no device is touched)
//   witness_merge_driver < DESCRIPTION
// DESCRIPTION, whitespace-separated: a tiny circuit, then the blocks of G ranks —
//   s_max m_I
//   K,  then K times:  subcircuitId name
//   P,  then P times:  the kind (index into the K entries) of placement q
//   E,  then E times:  row col X Y                       (permutation.json's entries; the effective permutation is made from them)
//   G,  then G times:  bad_cells bad_placements n_arithmetic bad_entries n_copy wires bad_public n_public failed failed_placement error
//                      (error: the bytes of the text as hex, or "-"), then min(n_arithmetic, 8) times  placement first_row bad_rows u v w,
//                      min(n_copy, 8) times  entry value source,  min(n_public, 8) times  index placement wire value instance
//                      (field values: 64 hex digits, most significant first)
// prints the merged report's JSON; or "error: <message>" (exit code 1)
#include <cstring>
#include <iostream>

#include "tkmk_witness_check.hpp"

using namespace tkmk;
using namespace tkmk::witness_check;

template <class T>
static T next() {
    T v;
    if (!(std::cin >> v)) throw Error("driver: the description ends early");
    return v;
}
static unsigned nibble(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    throw Error("driver: not a hex digit");
}
static ScalarField next_fr() {
    const std::string h = next<std::string>();
    if (h.size() != 64) throw Error("driver: a field value has 64 hex digits");
    ScalarField v{};
    for (size_t k = 0; k < 64; k++) v.limbs[7 - k / 8] |= nibble(h[k]) << (28 - 4 * (k % 8));
    return v;
}

int main() {
    try {
        SetupParams sp{};
        sp.s_max = next<size_t>(), sp.l_D = next<size_t>();   // l = 0: m_i() is l_D
        std::vector<SubcircuitInfo> infos(next<size_t>());
        for (SubcircuitInfo &i : infos) i.id = next<size_t>(), i.name = next<std::string>();
        WitnessLayout layout;
        layout.id.resize(next<size_t>());
        for (uint32_t &kind : layout.id) kind = next<uint32_t>();
        PermutationColumns cols;
        for (size_t e = next<size_t>(); e-- > 0;)
            cols.row.push_back(next<uint32_t>()), cols.col.push_back(next<uint32_t>()), cols.X.push_back(next<uint32_t>()), cols.Y.push_back(next<uint32_t>());
        const EffectivePermutation ep = effective_permutation(cols, sp.m_i(), sp.s_max);
        std::vector<ShardBlock> all(next<size_t>());
        for (ShardBlock &b : all) {
            std::memset(&b, 0, sizeof b);
            b.bad_cells = next<uint64_t>(), b.bad_placements = next<uint64_t>(), b.n_arithmetic = next<uint64_t>();
            b.bad_entries = next<uint64_t>(), b.n_copy = next<uint64_t>();
            b.wires = next<uint64_t>(), b.bad_public = next<uint64_t>(), b.n_public = next<uint64_t>();
            b.failed = next<uint32_t>(), b.failed_placement = next<uint32_t>();
            const std::string text = next<std::string>();
            if (text != "-")
                for (size_t k = 0; k + 1 < text.size() && k / 2 < sizeof b.error; k += 2) b.error[k / 2] = (char)(nibble(text[k]) << 4 | nibble(text[k + 1]));
            for (size_t k = 0; k < b.n_arithmetic && k < MAX_FINDINGS; k++) {
                ShardBlock::Arithmetic &f = b.arithmetic[k];
                f.placement = next<uint64_t>(), f.first_row = next<uint32_t>(), f.bad_rows = next<uint32_t>();
                f.u = next_fr(), f.v = next_fr(), f.w = next_fr();
            }
            for (size_t k = 0; k < b.n_copy && k < MAX_FINDINGS; k++) {
                ShardBlock::Copy &f = b.copy[k];
                f.entry = next<uint64_t>(), f.value = next_fr(), f.source = next_fr();
            }
            for (size_t k = 0; k < b.n_public && k < MAX_FINDINGS; k++) {
                ShardBlock::Public &f = b.pub[k];
                f.index = next<uint64_t>(), f.placement = next<uint64_t>(), f.wire = next<uint64_t>();
                f.value = next_fr(), f.instance = next_fr();
            }
        }
        Inputs in;
        in.sp = &sp, in.infos = &infos, in.layout = &layout, in.perm = &ep;
        Report rep;
        merge(in, all, rep);
        std::cout << rep.to_json() << "\n";
        return 0;
    } catch (const std::exception &e) {
        std::cout << "error: " << e.what() << "\n";
        return 1;
    }
}
