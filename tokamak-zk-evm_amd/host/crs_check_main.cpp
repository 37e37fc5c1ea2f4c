// crs_check_main.cpp — `crs-check`: is the reference string of a directory well formed for a circuit?  (host/tkmk_crs_audit.hpp)
//   crs-check --crs DIR [--subcircuit-library DIR] [--circuit] [--locate]
// Reads <lib>/setupParams.json and <crs>/combined_sigma.tkcrs or combined_sigma.rkyv, as `prove` does; without --subcircuit-library the
// library is resolved the way host/tkmk_args.hpp describes.  --circuit adds the table checks of the gamma / eta / delta tables against the
// circuit (reads <lib>/subcircuitInfo.json and <lib>/r1cs/ as well; one more stderr line per table).  No reference counterpart: the reference downloads its CRS at install
// (setup/mpc-setup/src/drive_upload.rs) and checks it inside the ceremony only.
// --locate: a structural check that fails goes on to name the record (the locate pass of host/tkmk_crs_audit.hpp); with --circuit it covers
// the tables as well, without it xy_powers only.  One more stderr line per finding: `crs-check: located <section>[<index>] (row r, col c)`
// with `, and at least one more` where the section still fails without the record, followed by the finding's sentence; a failure that is
// not a record's (a wrong sigma_2.y) is that sentence alone.  The verdict line and the exit status are what they are without it.
// stdout: the directory lines, then `true` or `false` as the LAST line, as bin/verify prints its verdict.  stderr: one line per section
// (points, infinity, not reduced, off the curve, outside the subgroup), the steps' verdicts and times, and the reason for `false`.
// Exit status 0 after either verdict; 1 when an input cannot be read or no device is present; 2 for a usage error.
#include <cstdio>
#include <string>

#include "tkmk_args.hpp"
#include "tkmk_crs_audit.hpp"

using namespace tkmk;

static const char *USAGE =
    "Usage: crs-check --crs <PATH> [--subcircuit-library <PATH>] [--circuit] [--locate]\n"
    "  --crs                 CRS directory containing combined_sigma.rkyv (or combined_sigma.tkcrs)\n"
    "  --subcircuit-library  Subcircuit library directory produced by the QAP compiler (default: see host/tkmk_args.hpp)\n"
    "  --circuit             Also check the gamma / eta / delta tables against the circuit of the library (reads its r1cs/ files)\n"
    "  --locate              When a structural check fails, go on to name the record that breaks it (xy_powers; with --circuit the tables too)\n";

int main(int argc, char **argv) {
    args::Spec spec{{"--crs", "--subcircuit-library"}, {"--circuit", "--locate"}};
    args::Parsed a = args::parse(argc, argv, spec);
    if (a.help) {
        fputs(USAGE, stdout);
        return 0;
    }
    if (a.version) {
        printf("crs-check %s\n", TKMK_BACKEND_INTERFACE_VERSION);
        return 0;
    }
    if (a.error.empty() && !a.has("--crs")) a.error = "the following required arguments were not provided: --crs <PATH>";
    if (!a.error.empty()) {
        fprintf(stderr, "error: %s\n\n%s", a.error.c_str(), USAGE);
        return 2;
    }
    try {
        const std::string lib_dir = args::resolve_subcircuit_library(a);
        printf("Subcircuit library: %s\n", lib_dir.c_str());
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, "no HIP device (the MI355X backend has no CPU fallback)");
        printf("Checking the reference string...\n");
        fflush(stdout);
        crs_audit::Report rep;
        std::string container;
        const bool ok = crs_audit::audit_files(lib_dir, a.get("--crs"), rep, &container, a.flag("--circuit"), a.flag("--locate"));
        fprintf(stderr, "crs-check: %s\n", container.c_str());
        auto word = [](int v) { return v < 0 ? "not reached" : v ? "ok" : "FAILED"; };
        for (const crs_audit::SectionReport &s : rep.sections)
            fprintf(stderr, "crs-check: %-30s %10llu points, %llu infinity, %llu not reduced, %llu off the curve, %llu outside the subgroup\n", s.name.c_str(),
                    (unsigned long long)s.r.n_checked, (unsigned long long)s.r.n_infinity, (unsigned long long)s.r.n_noncanonical,
                    (unsigned long long)s.r.n_off_curve, (unsigned long long)s.r.n_not_in_subgroup);
        fprintf(stderr, "crs-check: g2 points %s, anchors %s, powers along Y %s, powers along X %s\n", word(rep.g2), word(rep.anchors), word(rep.ratio_y),
                word(rep.ratio_x));
        fprintf(stderr, "crs-check: upload %.3f s, membership %.3f s, g2 %.3f s, four MSMs %.3f s, pairings %.3f s, total %.3f s\n", rep.upload_s, rep.membership_s,
                rep.g2_s, rep.msm_s, rep.pairing_s, rep.total_s);
        if (rep.circuit >= 0) {
            for (const crs_audit::TableReport &t : rep.tables)
                fprintf(stderr, "crs-check: table %-19s %10llu points, %s\n", t.name.c_str(), (unsigned long long)t.points,
                        !t.ok ? "FAILED" : t.points ? "ok" : "ok (empty: vacuously true)");
            fprintf(stderr, "crs-check: tables: library %.3f s, grids %.3f s, MSMs %.3f s, pairings %.3f s\n", rep.t_library_s, rep.t_grids_s, rep.t_msm_s,
                    rep.t_pairing_s);
        }
        if (!ok) fprintf(stderr, "crs-check: %s\n", rep.reason.c_str());
        for (const crs_audit::Finding &f : rep.located) {
            if (f.index < 0) {
                fprintf(stderr, "crs-check: %s: %s\n", f.check.c_str(), f.what.c_str());
                continue;
            }
            std::string where = f.row >= 0 ? " (row " + std::to_string(f.row) + ", col " + std::to_string(f.col) + ")" : std::string();
            fprintf(stderr, "crs-check: located %s[%lld]%s%s: %s\n", f.section.c_str(), (long long)f.index, where.c_str(), f.more ? ", and at least one more" : "",
                    f.what.c_str());
        }
        if (rep.locate) fprintf(stderr, "crs-check: locate: %llu pairing products, %.3f s\n", (unsigned long long)rep.locate_products, rep.locate_s);
        printf("%s\n", ok ? "true" : "false");
        return 0;
    } catch (const std::exception &e) {
        fflush(stdout);
        fprintf(stderr, "crs-check: %s\n", e.what());
        return 1;
    }
}
