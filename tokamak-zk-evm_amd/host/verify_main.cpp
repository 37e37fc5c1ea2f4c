// verify_main.cpp — native `verify` with the reference binary's argument surface (packages/backend/verify-rust/src/main.rs:8-69):
//   verify --crs DIR --synthesizer-stat DIR --preprocess DIR --proof DIR [--subcircuit-library DIR]
// which is what tokamak-cli sends (`backendVerifyArgs`, packages/cli/src/cli.ts:548-559); without --subcircuit-library the library is
// resolved the way host/tkmk_args.hpp describes.  Reads <lib>/setupParams.json, <synthesizer-stat>/instance.json, <crs>/sigma_verify.json,
// <preprocess>/preprocess.json, <proof>/proof.json (host/tkmk_verify.hpp).
// stdout: "Verifier initialization...", "Verifying the proof...", then `true` or `false` as the LAST line — the line the CLI parses
// (cli.ts:504-509).  Exit status 0 after either verdict (the reason for `false` goes to stderr); 1 with the reference's message on stderr
// when an input cannot be read or parsed; 2 for a usage error.
// Host-only: no GPU, no ROCm runtime, no libtkmk_hip.so.  The root-of-unity generator is TKMK_FR_ROOT_GENERATOR or the declared default
// (sigma_verify.json cannot tell which one its reference string was made under: host/tkmk_verify.hpp); stderr names the one used.
#include <cstdio>
#include <string>

#include "tkmk_args.hpp"
#include "tkmk_verify.hpp"

using namespace tkmk;

static const char *USAGE =
    "Usage: verify --crs <PATH> --synthesizer-stat <PATH> --preprocess <PATH> --proof <PATH> [--subcircuit-library <PATH>]\n"
    "  --crs               CRS output directory containing sigma_verify.json\n"
    "  --synthesizer-stat  Synthesizer output directory containing verification inputs\n"
    "  --preprocess        Preprocess output directory containing preprocess.json\n"
    "  --proof             Proof output directory containing proof.json\n"
    "  --subcircuit-library  Subcircuit library directory produced by the QAP compiler (default: see host/tkmk_args.hpp)\n";

int main(int argc, char **argv) {
    args::Spec spec{{"--crs", "--synthesizer-stat", "--preprocess", "--proof", "--subcircuit-library"}, {}};
    args::Parsed a = args::parse(argc, argv, spec);
    if (a.help) {
        fputs(USAGE, stdout);
        return 0;
    }
    if (a.version) {
        printf("verify %s\n", TKMK_BACKEND_INTERFACE_VERSION);
        return 0;
    }
    if (a.error.empty()) {
        std::string missing;
        for (const char *k : {"--crs", "--synthesizer-stat", "--preprocess", "--proof"})
            if (!a.has(k)) missing += std::string(missing.empty() ? "" : ", ") + k + " <PATH>";
        if (!missing.empty()) a.error = "the following required arguments were not provided: " + missing;
    }
    if (!a.error.empty()) {
        fprintf(stderr, "error: %s\n\n%s", a.error.c_str(), USAGE);
        return 2;
    }
    try {
        const std::string lib_dir = args::resolve_subcircuit_library(a);
        printf("Subcircuit library: %s\n", lib_dir.c_str());
        printf("Verifier initialization...\n");
        fflush(stdout);
        verify::Inputs in;
        in.sp = verify::read_shape(lib_dir);
        verify::validate_shape(in.sp);
        in.a_pub = verify::read_instance(a.get("--synthesizer-stat"), in.sp);
        verify::read_sigma_verify(a.get("--crs"), in);
        verify::read_preprocess(a.get("--preprocess"), in);
        verify::read_proof(a.get("--proof"), in);
        printf("Verifying the proof...\n");
        fflush(stdout);
        verify::Report rep;
        const bool ok = verify::verify_loaded(in, 0, rep);
        fprintf(stderr, "verify: root-of-unity generator %u\n", rep.generator);
        if (!ok) fprintf(stderr, "verify: %s\n", rep.reason.c_str());
        printf("%s\n", ok ? "true" : "false");
        return 0;
    } catch (const std::exception &e) {
        fflush(stdout);
        fprintf(stderr, "verify: %s\n", e.what());
        return 1;
    }
}
