/* tkmk_prover.h — C ABI of the resident prover (libtkmk_prover.so): the process/CLI boundary of `prove` and `preprocess`
 *  as library calls, for a host that produces many proofs of one circuit.
 *
 * Replaces, per call:
 *   tkmk_prover_open      the circuit-static part of Prover::init  (packages/backend/prove/src/lib.rs:675-835: setupParams.json,
 *                         subcircuitInfo.json, r1cs/subcircuit{id}.r1cs) + SigmaHolder::load (prove/src/sigma_source.rs:22-47:
 *                         <crs>/combined_sigma.rkyv; the flat <crs>/combined_sigma.tkcrs payload is accepted as a fast path)
 *                         + check_device (libs/src/utils/mod.rs:78-110)
 *   tkmk_prover_prove     main() of prove/src/main.rs:41-84: Prover::init on <synthesizer>/{placementVariables,permutation,
 *                         instance}.json, prove0..prove4 with the Fiat-Shamir transcript, <output>/proof.json in the
 *                         Solidity-verifier format (prove/src/lib.rs:452-513)
 *   tkmk_prover_close     process exit
 * A reference maintainer binds these three from Rust and keeps the `prove` argument surface.
 * One context per process and GPU; calls on one context must not overlap.  There is no CPU fallback: without a gfx950
 * device tkmk_prover_open returns TKMK_ERR_NO_DEVICE.  Errors: the tkmk_error code, text from tkmk_prover_last_error()
 * (the reference panics with the same messages). */
#ifndef TKMK_PROVER_H
#define TKMK_PROVER_H
#include "tkmk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tkmk_prover tkmk_prover;

typedef struct {          /* seconds */
    double parse_s;       /* the three synthesizer documents -> host arrays (all cores) */
    double upload_s;      /* witness + index arrays -> HBM */
    double build_s;       /* u, v, w, b, s0, s1, a_free on the device */
    double binding_s;     /* A_free, O_pub_free, O_mid, O_prv */
    double init_s;        /* Prover::init = the four above */
    double prove_s[5];    /* prove0 .. prove4 */
    double write_s;       /* proof.json */
    double total_s;
} tkmk_prove_timing;

/* Loads the circuit-static state.  Because the context is meant to stay, xy_powers is expanded once into a precomputed commit
 * table (ICICLE's msm_precompute_bases; 20-bit windows, 13 x the table in HBM: 21 GB for the 2^24-point CRS of BASELINE.json
 * configs[3]) so that every large commit costs 13 instead of 16 bucket additions per point; commitments are bit-identical either
 * way.  Environment: TKMK_PROVER_TABLE_C=0 disables the table, 13..20 picks another window width.
 * Resident cost per circuit, in full (BASELINE.json configs[3], n = m_I = 4096, s_max = 1024; the production shape s_max = 256 is a
 * quarter of each): the commit table 21 GB; the Lagrange-basis twin of the n x s_max grid in the same 13-level form 5.2 GB; its prefix
 * sums in prove1's walk order 5.2 GB; the binding tables 4.2 GB; the subcircuit library and the NTT domain < 1 GB — 36 GB of the 288 —
 * and 7.6 s at open (2.7 s table expansion, 3.3 s group NTT behind the Lagrange table, 1.3 s prefix sums and their expansion; production
 * shape 1.9 s).  TKMK_PROVER_LAGRANGE=0 drops the second and third items (U, V, W, B, R are then committed from coefficients).  A
 * sharded context (tkmk_prover_open_sharded) keeps 1 / G of the first three per GPU and does 1 / G of their one-time work.
 * THE ROOT OF UNITY IS IDENTIFIED FROM THE CRS, not assumed (tkmk.h: TKMK_BLS12_381_FR_ROOT_GENERATOR, tkmk_crs_identify_root): right after
 * xy_powers is uploaded, and before anything that depends on omega is built, lagrange_KL is recomputed from the m_I x s_max corner of
 * xy_powers under the generator in effect and under the other of {5, 7} — one plain-window MSM of m_I * s_max points and one scalar grid
 * per candidate (DESIGN.md section 5 has the measured cost).  Exactly one reproduces the CRS's record: if it is not the generator in
 * effect, the process-wide NTT domain is released and the generator replaced (tkmk_ntt_set_root_generator) — refused with
 * TKMK_ERR_INVALID_ARGUMENT while ANOTHER prover context of the process is open, since that one was built under the generator in effect.
 * None does: TKMK_ERR_INVALID_ARGUMENT, the message names every generator tried; no context is made.  Both do (m_I <= 2 and s_max <= 2):
 * the generator in effect stays.  TKMK_FR_ROOT_GENERATOR=<g> in the environment PINS the convention: that generator alone is tried.
 * tkmk_prover_root_generator tells which generator a context runs under.
 * THE RECORDS OF THE CRS ARE TAKEN ON FAITH unless TKMK_PROVER_CHECK_CRS=1 is in the environment: then the audit of tkmk_crs_audit_files
 * (below) runs on the payload just loaded, before anything is built from it (its own upload of every section: seconds at the production
 * shape), and a reference string that fails is refused with TKMK_ERR_INVALID_ARGUMENT — the message names the
 * section, the index and the reason; no context is made.  Unset or 0, open does exactly what it did before the audit existed.
 * TKMK_PROVER_CHECK_CRS=2 runs the audit of tkmk_crs_audit_circuit_files instead: the same, then the gamma / eta / delta tables against the
 * circuit of subcircuit_library_dir (which must hold subcircuitInfo.json and r1cs/); a table that fails is named in the message.
 * tkmk_prover_open_sharded does NOT read the variable (every rank would audit the whole file): audit the files once, with
 * tkmk_crs_audit_files or bin/crs-check, before the ranks start. */
tkmk_error tkmk_prover_open(const char *subcircuit_library_dir, const char *crs_dir, tkmk_prover **out);
/* ONE proof over the G GPUs of a node (the reference is single-device, so nothing is replaced).  G is a power of
 * two, at most min(n, m_I, s_max).  Rank r of the communicator `comm` (a tkmk_comm of include/tkmk_dist.h, made by the host: one process
 * per GPU over RCCL) holds the COLUMNS iy = r mod G of everything: of every commit table — xy_powers, the Lagrange-basis tables and their
 * prefix sums: resident HBM and the work at open (table expansion AND the group transforms behind the Lagrange tables) divide by G — and
 * of every coefficient matrix of a proof, so that the divisions, window sums and shifts along X, both passes of the vanishing division
 * and the commits are local to a rank; evaluations on the large domains live in row slabs, and a bivariate transform crosses between
 * the two layouts with ONE all-to-all.  The witness side divides by placement (a placement is a column of u, v, w, b): a rank converts,
 * uploads, evaluates and routes its own placements only.  Replicated: the Fiat-Shamir transcript (every rank derives the same challenges
 * from the same gathered commitments) and the small polynomials built from host values.  Exchanges per proof: one all-gather per commit
 * batch (144 B per commitment + a status block), one all-to-all per transform, a ring shift per Y-shifted term, all-gathers of a few
 * values (evaluation partials, remainder rows), one broadcast of rank 0's blinding scalars; DESIGN.md section 6 counts them.
 * The root-of-unity check of tkmk_prover_open runs on every rank over its own columns of the corner; one all-gather carries the partial
 * sums, every rank adds them and reaches the same decision: an adoption or a refusal is every rank's.
 * Every rank must call _open_sharded and then every _prove / _prove_ex with the same arguments; every rank gets the same proof, byte for
 * byte the one the single-GPU context gives for the same blinding scalars (tests/test_gpu_sharded_prover.py, G = 2, 4, 8 over the
 * loopback transport); RANK 0 ALONE writes <output_dir>/proof.json (temporary file + rename), after all ranks agreed that they
 * finished.  An input error only one rank can see is agreed on and reported by all; a rank that fails for a reason its peers cannot share
 * (memory, device, transport) aborts the communicator (tkmk_comm_abort) so that they fail instead of waiting — the contexts of an aborted
 * communicator can only be closed.  libtkmk_dist.so must be in the process (it is: the host made `comm` with it). */
tkmk_error tkmk_prover_open_sharded(void *comm, const char *subcircuit_library_dir, const char *crs_dir, tkmk_prover **out);
int tkmk_prover_world_size(const tkmk_prover *p);   /* 1 for a context made by tkmk_prover_open */
/* output_dir may be NULL (no file is written); proof_json_out (optional) receives a malloc'ed copy of the document, to be
 * released with tkmk_prover_free_string.  testing_mixer_json: NULL in production (blinding scalars from getrandom());
 * a path to a JSON document with fixed blinding scalars makes the proof deterministic — for differential tests only,
 * a proof made with known blinding scalars is not zero-knowledge. */
tkmk_error tkmk_prover_prove(tkmk_prover *p, const char *synthesizer_dir, const char *output_dir, const char *testing_mixer_json,
                             tkmk_prove_timing *timing, char **proof_json_out);
/* The same with two switches for parity work and a record of what every commitment ran over.
 * flags: TKMK_PROVE_TEST_PARTS        prove4 commits Pi_AX, Pi_AY, Pi_CX, Pi_CY, Pi_B, M_X, N_X one by one and adds the points — the
 *                                     reference's own commit list (prove/src/lib.rs:2572-3184) — where the default adds the quotient
 *                                     polynomials first and commits Pi_X, Pi_Y once and N_X not at all (N_X = M_X);
 *        TKMK_PROVE_COEFFICIENT_BASIS U, V, W, B, R are committed from their coefficients (the reference's encode_poly) although the
 *                                     context holds the Lagrange-basis tables.
 * Neither changes a byte of the proof.  commit_boxes_json_out (optional, malloc'ed, tkmk_prover_free_string): a JSON array
 * [{"name", "x", "y", "basis": "coeff" | "evals"}] in commit order — (x_degree + 1) x (y_degree + 1) of encode_poly
 * (libs/src/iotools/mod.rs:2055-2060), the `msm=AxB` column of the reference's timing reports
 * (prove/optimization/timing.local.cpu.current.md "Encode Details"); pinned by tests/golden/encode_dims.json. */
#define TKMK_PROVE_TEST_PARTS 1
#define TKMK_PROVE_COEFFICIENT_BASIS 2
tkmk_error tkmk_prover_prove_ex(tkmk_prover *p, const char *synthesizer_dir, const char *output_dir, const char *testing_mixer_json, int flags,
                                tkmk_prove_timing *timing, char **proof_json_out, char **commit_boxes_json_out);
tkmk_error tkmk_prover_close(tkmk_prover *p);
void tkmk_prover_free_string(char *s);
const char *tkmk_prover_last_error(void);   /* message of the last failed call on this thread */
/* where the context's reference string came from: "combined_sigma.rkyv" or "combined_sigma.tkcrs" */
const char *tkmk_prover_crs_source(const tkmk_prover *p);
/* the root-of-unity generator the context runs under: the one its reference string was made under (see tkmk_prover_open) */
uint32_t tkmk_prover_root_generator(const tkmk_prover *p);

/* ---- The verifier (verify-rust/src/lib.rs: Verifier::init + verify_snark; host/tkmk_verify.hpp, host/tkmk_pairing.hpp) ----
 * HOST ONLY: none of the three calls below touches a device, so they also work where there is none; a verification is ~25 G1 scalar
 * multiplications, one ten-pair Miller loop and one final exponentiation, plus the membership checks of 26 G1 and 10 G2 points: about
 * 0.1 s on one core.
 *
 * *is_one = 1 iff prod_i e(p[i], q[i]) = 1 for BLS12-381 (n = 0: 1; a pair with the all-zero record = infinity on either side
 * contributes 1).  Every point is checked first: a coordinate >= p, a point off its curve or outside the subgroup of order r gives
 * TKMK_ERR_INVALID_ARGUMENT, and tkmk_prover_last_error() names the index and the reason. */
tkmk_error tkmk_pairing_product_is_one(const tkmk_g1_affine *p, const tkmk_g2_affine *q, size_t n, int *is_one);
/* What the reference's `verify` does with the same five directories: reads <lib>/setupParams.json, <synthesizer>/instance.json,
 * <crs>/sigma_verify.json, <preprocess>/preprocess.json, <proof>/proof.json, replays the transcript, draws kappa2 from getrandom() and
 * decides the ten-pairing equation.  *ok = 1 / 0 is the decision, with TKMK_SUCCESS either way: 0 also for a well-formed document that
 * holds an invalid group element (off the curve, outside the subgroup, coordinate >= p) or an all-zero Sigma2.  A document that cannot
 * be read or parsed is an error (the message names the file).
 * root_generator: the generator g (omega_{2^32} = g^((r-1)/2^32)) the reference string was made under; 0 = the one in effect:
 * TKMK_FR_ROOT_GENERATOR, else TKMK_BLS12_381_FR_ROOT_GENERATOR.  sigma_verify.json cannot tell which it was, so exactly this one is
 * used and no other is tried.  report_json_out (optional, tkmk_prover_free_string): {"generator", "ok", "reason", "thetas": [3], "kappa0",
 * "chi", "zeta", "kappa1", "a_eval"} — scalars as 0x + 64 hex digits; the challenges are absent when the decision fell before them. */
tkmk_error tkmk_verify_files(const char *subcircuit_library_dir, const char *crs_dir, const char *synthesizer_dir, const char *preprocess_dir,
                             const char *proof_dir, uint32_t root_generator, int *ok, char **report_json_out);
/* The self-check of a resident context: the same decision with G, x, y, lagrange_KL and Sigma2 taken from the context's own reference
 * string (the G1Singles and G2Points sections it was opened with) and the generator the context runs under
 * (tkmk_prover_root_generator) — a context that adopted generator 7 at open verifies its own proofs with no environment set.  Pure host
 * work on host copies: no device call, no change to the proving state, no collective — every rank of a sharded context may call it. */
tkmk_error tkmk_prover_verify(tkmk_prover *p, const char *synthesizer_dir, const char *preprocess_dir, const char *proof_dir, int *ok,
                              char **report_json_out);

/* ---- Batch verification: n proofs of ONE circuit against ONE reference string (verify_batch of host/tkmk_verify.hpp) ----
 * Every proof is checked against the same ten G2 points and every G1 input of its ten pairs is a linear combination of named points, so
 * with fresh random weights r_k the product over a set of proofs collapses to ten pairs again: prod_j e(sum_k r_k P_{k,j}, Q_j) = 1.  A
 * batch of honest proofs costs ONE product of ten pairings, ten multi-scalar multiplications over about 22 n points and one membership
 * pass, instead of n products.
 *   verdicts    PER PROOF, never per batch: ok_each[k] = 1 / 0 equals what tkmk_verify_files says for item k alone, *ok_all = 1 iff all are
 *               1.  If the fold of all items fails, the set is halved and re-folded until the false items stand alone: at most
 *               1 + 2 b ceil(log2 n) products for b false items; the report's "products" is the count.
 *   weights     r_k in [1, 2^128) from getrandom(), drawn after every input is loaded, new for every fold (re-folds included), never
 *               derived from a counter or a seed expansion: a set holding a false proof passes a fold with probability <= 2^-128.
 *   membership  is never folded (E(Fp) has a cofactor; a random combination does not see a small-order component): every distinct G1
 *               record is checked, an item with a bad one is false with the single verifier's reason and enters no fold.  Records shared
 *               by many items (G, sigma_1.x, sigma_1.y, lagrange_KL; s0, s1, O_pub_fix of items with the same preprocess) are checked
 *               once.  Sigma2 is checked once; an all-zero Sigma2, a bad G2 point or one at infinity makes every item false with that reason.
 *   route       the caller's choice, no hidden size threshold.  TKMK_VERIFY_ROUTE_HOST: pure host work on TKMK_HOST_THREADS threads, no
 *               device call.  TKMK_VERIFY_ROUTE_DEVICE: the records are uploaded once, ONE tkmk_g1_check call does the membership pass and
 *               one tkmk_msm_segmented call per fold (and one tkmk_msm_multi_ex call for the slot jobs too long for it) the ten sums
 *               (host/tkmk_verify_device.hpp; the report counts both: "segmented_jobs", "pipeline_jobs"); the pairing stays on the host.  It runs on
 *               the default stream in its own buffers, takes turns with the prover contexts of the process, and reads and changes no
 *               library or context state (NTT domain, generator in effect, commit tables).  Without a device: TKMK_ERR_NO_DEVICE.  For
 *               ONE item the two routes cost the same; from a few items on the device route is the faster one.
 *   errors      n = 0 is TKMK_ERR_INVALID_ARGUMENT (a vacuous "all true" does not exist); a document that cannot be read or parsed is an
 *               error whose message names the item index and the file, and no verdict is given.
 * report_json_out (optional, tkmk_prover_free_string): {"generator", "ok", "n", "route": "host" | "device", "products", "segmented_jobs", "pipeline_jobs", "items": [one
 * report of tkmk_verify_files per item], "seconds": {"parse", "membership", "fold", "pairings", "total"}}.
 * NOT covered: batches across different reference strings or circuits, BN254, a device route for sharded contexts. */
typedef struct {
    const char *synthesizer_dir, *preprocess_dir, *proof_dir;
} tkmk_verify_item;
#define TKMK_VERIFY_ROUTE_HOST 0
#define TKMK_VERIFY_ROUTE_DEVICE 1
tkmk_error tkmk_verify_batch_files(const char *subcircuit_library_dir, const char *crs_dir, const tkmk_verify_item *items, size_t n,
                                   uint32_t root_generator, int route, uint8_t *ok_each /* n */, int *ok_all, char **report_json_out);
/* The same against the context's own reference string and generator (as tkmk_prover_verify); the Sigma2 check is made once per context and
 * kept.  TKMK_VERIFY_ROUTE_DEVICE on a context from tkmk_prover_open_sharded is TKMK_ERR_INVALID_ARGUMENT: sharded ranks keep the host
 * route, which needs no collective — every rank may call it. */
tkmk_error tkmk_prover_verify_batch(tkmk_prover *p, const tkmk_verify_item *items, size_t n, int route, uint8_t *ok_each, int *ok_all,
                                    char **report_json_out);


/* ---- The audit of a reference string (host/tkmk_crs_audit.hpp; needs a device) ----
 * Reads <lib>/setupParams.json and <crs>/combined_sigma.tkcrs or .rkyv (as tkmk_prover_open does) and decides whether the CRS is well
 * formed: *ok = 1 iff
 *   every record of every G1 section (xy_powers, gamma_inv_o_inst, eta_inv_li_o_inter_alpha4_kj, delta_inv_li_o_prv, the three small delta
 *   tables, the six single points) is canonical, on the curve and in the subgroup of order r (tkmk_g1_check, one upload per section),
 *   no record of xy_powers is infinity, and the ten G2 points pass the host's checks;
 *   xy_powers[0] = G, xy_powers[1] = sigma_1.y, xy_powers[rs_y] = sigma_1.x;
 *   xy_powers is the table [x^a y^b]G: for one grid rho of random scalars, four MSMs over views of the uploaded table (one
 *   tkmk_msm_multi_ex call) and two pairing products, e(R_y, H) e(-L_y, [y]H) = 1 and e(R_x, H) e(-L_x, [x]H) = 1 — skipped when
 *   membership failed.  rho expands from a 64-bit seed drawn from getrandom() AT CALL TIME, after the file is fixed; the expansion
 *   (splitmix64) is not a cryptographic generator.  TKMK_CRS_AUDIT_SEED=<n> fixes the seed in libtkmk_prover_testing.so only.
 * This entry gives the gamma / eta / delta tables membership only: their structure depends on the circuit polynomials, which
 * tkmk_crs_audit_circuit_files (below) reads.
 * TKMK_SUCCESS after either verdict; a file that cannot be read or does not match setupParams.json is an error, and so is a machine
 * without a device (TKMK_ERR_NO_DEVICE).  report_json_out (optional, tkmk_prover_free_string): {"ok", "reason", "sections": [{"name",
 * "points", "infinity", "noncanonical", "off_curve", "not_in_subgroup", "first_bad"}], "g2", "anchors", "ratio_y", "ratio_x", "seconds":
 * {"upload", "membership", "g2", "msm", "pairings", "total"}, "circuit", "tables", "table_seconds"} — null for a step that was not
 * reached, first_bad null when none; the last three keys are null from this entry.  The three keys of the locate pass follow
 * (tkmk_crs_audit_files_ex below; from this entry "located": null, "locate_products": 0). */
tkmk_error tkmk_crs_audit_files(const char *subcircuit_library_dir, const char *crs_dir, int *ok, char **report_json_out);
/* The same contract, plus the table checks against the circuit: needs <lib>/subcircuitInfo.json and <lib>/r1cs/subcircuit{id}.r1cs as well
 * (a missing or malformed file is an error return, not a verdict).  After everything above has passed — the table checks rest on
 * xy_powers being right, which stays on the device through them — every record of the seven G1 tables is tied to the circuit:
 *   gamma, eta, delta   a random combination of the table (weights a_j per flattened wire, b_i per placement column: the rank-one grid
 *                       a_j b_i) against MSMs over xy_powers of the circuit's own polynomials — tkmk_r1cs_library_mix and tkmk_fr_outer build
 *                       the evaluation grids, tkmk_bintt turns them into coefficients — through one pairing product per table against
 *                       [gamma]H, [eta]H, [delta]H and [alpha^k]H;
 *   delta_small         the 9 + 2 + 12 records of the three small delta tables against differences of xy_powers records (an infinity
 *                       record among them is a failure);
 *   alpha_chain         sigma_2.alpha .. alpha4 are powers of one alpha;
 *   singles             sigma_1.delta and sigma_1.eta are [delta]G and [eta]G for the delta and eta of sigma_2.
 * The root of unity the Lagrange bases are taken over is identified from the CRS first, as tkmk_prover_open does (a CRS made under
 * generator 7 audits as one made under 5; adopting it is process-wide).  Together this fixes all seven G1 tables and the single points,
 * and sigma_2 except that gamma, delta, eta are tied to the tables only, not to each other.  NOT covered: sigma_preprocess.rkyv, the
 * sharded open, BN254.  Which record of a failed table is wrong is what TKMK_CRS_AUDIT_LOCATE (below) finds.  The seed caveat above holds unchanged.
 * Report: "circuit" true / false (null when an earlier step failed), "tables": [{"name", "points", "ok"}] for gamma, eta, delta,
 * delta_small, alpha_chain, singles (an empty table is vacuously ok with 0 points), "table_seconds": {"library", "grids", "msm", "pairings"}. */
tkmk_error tkmk_crs_audit_circuit_files(const char *subcircuit_library_dir, const char *crs_dir, int *ok, char **report_json_out);
/* The audit by flags: 0 is tkmk_crs_audit_files, TKMK_CRS_AUDIT_CIRCUIT is tkmk_crs_audit_circuit_files (both are calls of this entry), and
 * TKMK_CRS_AUDIT_LOCATE adds the locate pass to either: a STRUCTURAL check that fails (a membership failure names its record already) goes
 * on to name the record, or says that the failure is not a record's.  Every equation of the audit is linear in its weights, so a failing
 * check splits into two half-checks over the same scalars — nothing new is drawn — and the first bad record is about log2(N) evaluations
 * of an equation that exists already away; one more evaluation with that record's terms set aside decides `more`.
 *   xy_powers (ratio_y / ratio_x false; without TKMK_CRS_AUDIT_CIRCUIT this is all the pass covers)   per failed direction first
 *       e(sigma_1.y, H) = e(G, sigma_2.y) (resp. x): if that fails, sigma_2 is at fault and no record is searched for.  Else the rectangle
 *       of relations is bisected, rows then columns, over views of the uploaded table; the record named is the one that the first
 *       failing relations of both directions touch, else the relation is reported with "index": null.
 *   gamma, eta, delta   the table's equation restricted to a range of rows (eta / delta: then to a range of placement columns of the row
 *       found); the last step is the equation of one record, an exact statement.  A step costs one evaluation of the table's equation.
 *   delta_small, alpha_chain, singles   the records one at a time.
 * A search runs only where the check's own prerequisites held.  With the flag clear the call is the entry without it: the same launches,
 * report text and reason; with it set and an honest CRS nothing extra runs.  tkmk_prover_open never locates (TKMK_PROVER_CHECK_CRS): run
 * this, or bin/crs-check --locate, after a refusal.  Not on a sharded prover, not for BN254; one record per check (the first in index order).
 * Report: three keys after all of the above — "located": null without the flag, [] when nothing was located, else in check order
 * [{"check": "ratio_y" | "ratio_x" | "gamma" | "eta" | "delta" | "delta_small" | "alpha_chain" | "singles", "section": the payload section,
 * "index", "row", "col" (null where they do not apply), "more": the section still fails without the record, "what": one sentence}];
 * "locate_products": pairing products spent locating; "locate_seconds".  "reason" keeps its text, the first finding's "what" appended.
 * TKMK_ERR_INVALID_ARGUMENT for an unknown flag bit. */
#define TKMK_CRS_AUDIT_CIRCUIT 1
#define TKMK_CRS_AUDIT_LOCATE 2
tkmk_error tkmk_crs_audit_files_ex(const char *subcircuit_library_dir, const char *crs_dir, uint32_t flags, int *ok, char **report_json_out);

/* ---- The witness check (host/tkmk_witness_check.hpp; needs a device and NO reference string) ----
 * Reads the library (<lib>/setupParams.json, subcircuitInfo.json, r1cs/) and the three per-proof documents of synthesizer_dir, puts the
 * witness on the device exactly as Prover::init does (the same code) and decides three sections, always all three: *ok = 1 iff
 *   arithmetic   every placement's variables satisfy its subcircuit's R1CS: u . v = w in every cell of the n x s_max evaluation grids
 *                (tkmk_witness_check_r1cs);
 *   copy         every entry {row, col, X, Y} of the effective permutation (the last writer of a cell wins, as in init) ties two equal
 *                interface values, b[row][col] = b[X][Y] (tkmk_witness_check_copy), and that map, extended by the identity on the
 *                cells no entry writes, is a bijection of the m_I x s_max cells;
 *   public       every public wire of placements 0..3 (the outputs of bufferPubOut, the inputs of bufferPubIn / bufferBlockIn /
 *                bufferEVMIn) equals the value of instance.json (a_pub_user ++ a_pub_block ++ a_pub_function) at its flattenMap index.
 * The verifier defines "wrong": *ok is what tkmk_prover_verify answers for the proof the prover makes from the same documents.
 * TKMK_SUCCESS after either verdict; an unreadable or malformed document is an error whose message names the file, and so is a machine
 * without a device (TKMK_ERR_NO_DEVICE).  report_json_out (optional, tkmk_prover_free_string): {"ok", "reason" (the first finding of
 * the first failing section, "" when ok), "arithmetic": {"ok", "placements", "bad_placements", "bad_cells", "first": [{"placement",
 * "subcircuitId", "name", "first_row", "bad_rows", "u", "v", "w"}]}, "copy": {"ok", "entries", "bijection", "hit_twice" ({"row", "col"},
 * present when not a bijection), "bad_entries", "first": [{"entry", "row", "col", "X", "Y", "value", "source"}]}, "public": {"ok", "wires",
 * "bad", "first": [{"index", "placement", "wire", "value", "instance"}]}, "seconds": {"parse", "upload", "build", "check", "total"}} — at
 * most 8 findings per section, field values as 0x + 64 hex digits.  Sharded contexts: tkmk_prover_check_witness_sharded below.  Not
 * covered: a sharded form of THIS entry or of bin/witness-check (there is no sharded context without a reference string), BN254, WHICH
 * variable of a failing row is wrong. */
tkmk_error tkmk_witness_check_files(const char *subcircuit_library_dir, const char *synthesizer_dir, int *ok, char **report_json_out);
/* The same against a resident context's library (nothing is read from subcircuit_library_dir again): own device buffers, a turn on the
 * default stream like a proof, and nothing a later tkmk_prover_prove reads is changed.  This entry is NOT collective: on a context from
 * tkmk_prover_open_sharded it returns TKMK_ERR_INVALID_ARGUMENT (the copy section compares cells of different columns, which live on
 * different ranks) and the message names tkmk_prover_check_witness_sharded.
 * TKMK_PROVER_CHECK_WITNESS=1 in the environment makes tkmk_prover_prove[_ex] (and bin/prove) run the three sections inside init, on the
 * grids it has just built, before the binding commitments are issued: a witness that fails is refused with TKMK_ERR_INVALID_ARGUMENT,
 * tkmk_prover_last_error() carries the report's "reason", no proof.json is written and the context stays usable.  Unset or 0: nothing is
 * launched, nothing is downloaded and (sharded) nothing is exchanged.  A sharded context reads the variable too — every rank must run
 * with the same value: the check is the collective one below, a refusal is every rank's error with one and the same text, no rank writes
 * proof.json, and the communicator is not aborted (the outcome is replicated), so the contexts stay usable. */
tkmk_error tkmk_prover_check_witness(tkmk_prover *p, const char *synthesizer_dir, int *ok, char **report_json_out);
/* The check on a sharded context: COLLECTIVE — every rank calls it with the same arguments, every rank gets the same *ok and the same
 * report (byte for byte outside "seconds", the report of tkmk_prover_check_witness on a single-GPU context for the same documents).
 * arithmetic and public are local to the rank that holds the placement; for copy every rank packs the source values the permutation
 * asks of its columns, ONE tkmk_comm_all_gather_dev hands all of them to every rank (at most about one copy of b when the sources are
 * spread evenly: m_I * s_max * 32 bytes), each rank compares its own destination cells (tkmk_witness_check_copy_split), and ONE
 * tkmk_comm_all_gather_host merges the findings: two exchanges beyond the agreement on the parsed documents.  The contract is that of
 * tkmk_prover_check_witness otherwise: own device buffers, nothing a later proof reads is changed, an unreadable document is every
 * rank's error naming the file (the communicator lives on); a device or transport failure aborts the communicator, as in _prove.  On a
 * context from tkmk_prover_open it is tkmk_prover_check_witness.  Not covered: BN254, WHICH variable of a failing row is wrong, an
 * all-to-all in place of the all-gather. */
tkmk_error tkmk_prover_check_witness_sharded(tkmk_prover *p, const char *synthesizer_dir, int *ok, char **report_json_out);

#ifdef __cplusplus
}
#endif
#endif
