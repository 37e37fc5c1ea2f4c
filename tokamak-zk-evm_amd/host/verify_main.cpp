// verify_main.cpp — native `verify` with the reference binary's argument surface (packages/backend/verify-rust/src/main.rs:8-69):
//   verify --crs DIR --synthesizer-stat DIR --preprocess DIR --proof DIR [--subcircuit-library DIR]
// which is what tokamak-cli sends (`backendVerifyArgs`, packages/cli/src/cli.ts:548-559); without --subcircuit-library the library is
// resolved the way host/tkmk_args.hpp describes.  Reads <lib>/setupParams.json, <synthesizer-stat>/instance.json, <crs>/sigma_verify.json,
// <preprocess>/preprocess.json, <proof>/proof.json (host/tkmk_verify.hpp).
// stdout: "Verifier initialization...", "Verifying the proof...", then `true` or `false` as the LAST line — the line the CLI parses
// (cli.ts:504-509).  Exit status 0 after either verdict (the reason for `false` goes to stderr); 1 with the reference's message on stderr
// when an input cannot be read or parsed; 2 for a usage error.
//   verify --batch MANIFEST --crs DIR [--subcircuit-library DIR]
// many proofs of one circuit against one reference string (verify_batch of host/tkmk_verify.hpp, host route): MANIFEST is a JSON array of
// {"synthesizer-stat": DIR, "preprocess": DIR, "proof": DIR}.  stdout: the two progress lines, one "<index> true|false" line per item, and
// as the LAST line `true` iff every item is true; the reasons go to stderr with the index.  Exit status as above; --batch together with
// --proof, --preprocess or --synthesizer-stat is a usage error.
// Host-only: no GPU, no ROCm runtime, no libtkmk_hip.so.  The root-of-unity generator is TKMK_FR_ROOT_GENERATOR or the declared default
// (sigma_verify.json cannot tell which one its reference string was made under: host/tkmk_verify.hpp); stderr names the one used.
#include <cstdio>
#include <string>

#include "tkmk_args.hpp"
#include "tkmk_verify.hpp"

using namespace tkmk;

static const char *USAGE =
    "Usage: verify --crs <PATH> --synthesizer-stat <PATH> --preprocess <PATH> --proof <PATH> [--subcircuit-library <PATH>]\n"
    "       verify --batch <MANIFEST> --crs <PATH> [--subcircuit-library <PATH>]\n"
    "  --crs               CRS output directory containing sigma_verify.json\n"
    "  --synthesizer-stat  Synthesizer output directory containing verification inputs\n"
    "  --preprocess        Preprocess output directory containing preprocess.json\n"
    "  --proof             Proof output directory containing proof.json\n"
    "  --batch             JSON array of {\"synthesizer-stat\", \"preprocess\", \"proof\"} directories: one verdict line per item\n"
    "  --subcircuit-library  Subcircuit library directory produced by the QAP compiler (default: see host/tkmk_args.hpp)\n";

// --batch: the manifest is read before anything else of the batch, and a malformed one is an input error (exit status 1)
static int batch(const args::Parsed &a, const std::string &lib_dir) {
    std::vector<verify::BatchItem> items;
    try {
        const json::Value m = json::read_file(a.get("--batch"));
        for (const json::Value &e : m.items()) items.push_back({e.at("synthesizer-stat").as_string(), e.at("preprocess").as_string(), e.at("proof").as_string()});
    } catch (const std::exception &e) {
        throw Error("manifest " + a.get("--batch") + ": " + e.what());
    }
    printf("Verifying the proof...\n");
    fflush(stdout);
    verify::HostFolder folder;
    verify::BatchReport rep;
    const bool all = verify::verify_batch_files(lib_dir, a.get("--crs"), items, 0, folder, rep);
    fprintf(stderr, "verify: root-of-unity generator %u\n", rep.generator);
    fprintf(stderr, "verify: %zu items, %llu pairing products\n", items.size(), (unsigned long long)rep.products);
    for (size_t k = 0; k < rep.items.size(); k++) {
        if (!rep.items[k].ok) fprintf(stderr, "verify: item %zu: %s\n", k, rep.items[k].reason.c_str());
        printf("%zu %s\n", k, rep.items[k].ok ? "true" : "false");
    }
    printf("%s\n", all ? "true" : "false");
    return 0;
}

int main(int argc, char **argv) {
    args::Spec spec{{"--crs", "--synthesizer-stat", "--preprocess", "--proof", "--subcircuit-library", "--batch"}, {}};
    args::Parsed a = args::parse(argc, argv, spec);
    if (a.help) {
        fputs(USAGE, stdout);
        return 0;
    }
    if (a.version) {
        printf("verify %s\n", TKMK_BACKEND_INTERFACE_VERSION);
        return 0;
    }
    if (a.error.empty() && a.has("--batch")) {
        for (const char *k : {"--proof", "--preprocess", "--synthesizer-stat"})
            if (a.has(k) && a.error.empty()) a.error = std::string("the argument '--batch <MANIFEST>' cannot be used with '") + k + " <PATH>'";
        if (a.error.empty() && !a.has("--crs")) a.error = "the following required arguments were not provided: --crs <PATH>";
    } else if (a.error.empty()) {
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
        if (a.has("--batch")) return batch(a, lib_dir);
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
