// witness_check_main.cpp — `witness-check`: does the witness of a synthesizer directory satisfy the circuit, and if not, where?
// (host/tkmk_witness_check.hpp)
//   witness-check --synthesizer-stat DIR [--subcircuit-library DIR]
// Reads <lib>/setupParams.json, subcircuitInfo.json, r1cs/ and <synth>/placementVariables.json, permutation.json, instance.json; without
// --subcircuit-library the library is resolved the way host/tkmk_args.hpp describes.  Needs a device and NO reference string.  The
// reference has these diagnostics behind its `testing-mode` feature only (prove/src/lib.rs:916-1017, 1472-1518).
// stdout: the directory line, one line per section, then `true` or `false` as the LAST line, as bin/verify prints its verdict.  stderr:
// the findings (at most 8 per section) and the times.
// Exit status 0 after either verdict; 1 when an input cannot be read or no device is present; 2 for a usage error.
#include <cstdio>
#include <string>

#include "tkmk_args.hpp"
#include "tkmk_service.hpp"

using namespace tkmk;

static const char *USAGE =
    "Usage: witness-check --synthesizer-stat <PATH> [--subcircuit-library <PATH>]\n"
    "  --synthesizer-stat    Synthesizer output directory (placementVariables.json, permutation.json, instance.json)\n"
    "  --subcircuit-library  Subcircuit library directory produced by the QAP compiler (default: see host/tkmk_args.hpp)\n";

int main(int argc, char **argv) {
    args::Spec spec{{"--synthesizer-stat", "--subcircuit-library"}, {}};
    args::Parsed a = args::parse(argc, argv, spec);
    if (a.help) {
        fputs(USAGE, stdout);
        return 0;
    }
    if (a.version) {
        printf("witness-check %s\n", TKMK_BACKEND_INTERFACE_VERSION);
        return 0;
    }
    if (a.error.empty() && !a.has("--synthesizer-stat")) a.error = "the following required arguments were not provided: --synthesizer-stat <PATH>";
    if (!a.error.empty()) {
        fprintf(stderr, "error: %s\n\n%s", a.error.c_str(), USAGE);
        return 2;
    }
    try {
        const std::string lib_dir = args::resolve_subcircuit_library(a);
        printf("Subcircuit library: %s\n", lib_dir.c_str());
        fflush(stdout);
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, "no HIP device (the MI355X backend has no CPU fallback)");
        std::unique_ptr<ProverContext> ctx = ProverContext::open_circuit(lib_dir);
        witness_check::Report rep;
        const bool ok = ctx->check_witness(a.get("--synthesizer-stat"), rep);
        auto word = [](bool v) { return v ? "ok" : "FAILED"; };
        printf("arithmetic: %s (%zu placements, %zu failing, %llu failing cells)\n", word(rep.arithmetic.ok), rep.arithmetic.placements, rep.arithmetic.bad_placements,
               (unsigned long long)rep.arithmetic.bad_cells);
        printf("copy:       %s (%llu entries, %s, %llu failing)\n", word(rep.copy.ok), (unsigned long long)rep.copy.entries,
               rep.copy.bijection ? "a bijection" : "NOT a bijection", (unsigned long long)rep.copy.bad_entries);
        printf("public:     %s (%zu wires, %zu failing)\n", word(rep.pub.ok), rep.pub.wires, rep.pub.bad);
        fflush(stdout);
        for (const witness_check::ArithmeticFinding &f : rep.arithmetic.first)
            fprintf(stderr, "witness-check: arithmetic: placement %zu (subcircuit %zu, %s): %u failing row(s), first row %u: u = %s, v = %s, w = %s\n", f.placement,
                    f.subcircuit_id, f.name.c_str(), f.bad_rows, f.first_row, witness_check::fr_hex(f.u).c_str(), witness_check::fr_hex(f.v).c_str(),
                    witness_check::fr_hex(f.w).c_str());
        if (!rep.copy.bijection)
            fprintf(stderr, "witness-check: copy: not a bijection: cell (row %u, col %u) is the image of two cells\n", rep.copy.twice_row, rep.copy.twice_col);
        for (const witness_check::CopyFinding &f : rep.copy.first)
            fprintf(stderr, "witness-check: copy: entry %llu (row %u, col %u) = %s, its source (X %u, Y %u) = %s\n", (unsigned long long)f.entry, f.row, f.col,
                    witness_check::fr_hex(f.value).c_str(), f.X, f.Y, witness_check::fr_hex(f.source).c_str());
        for (const witness_check::PublicFinding &f : rep.pub.first)
            fprintf(stderr, "witness-check: public: index %zu (placement %zu, wire %zu) = %s, instance.json has %s\n", f.index, f.placement, f.wire,
                    witness_check::fr_hex(f.value).c_str(), witness_check::fr_hex(f.instance).c_str());
        fprintf(stderr, "witness-check: parse %.3f s, upload %.3f s, build %.3f s, check %.3f s, total %.3f s\n", rep.parse_s, rep.upload_s, rep.build_s, rep.check_s,
                rep.total_s);
        if (!ok) fprintf(stderr, "witness-check: %s\n", rep.reason.c_str());
        printf("%s\n", ok ? "true" : "false");
        return 0;
    } catch (const std::exception &e) {
        fflush(stdout);
        fprintf(stderr, "witness-check: %s\n", e.what());
        return 1;
    }
}
