// prover_abi.cpp — libtkmk_prover.so: the C ABI of include/tkmk_prover.h over host/tkmk_service.hpp (ProverContext).
// Built twice: libtkmk_prover.so (production: blinding scalars always from getrandom(), a testing_mixer_json argument is refused)
// and, with -DTKMK_TESTING_MODE, libtkmk_prover_testing.so for the differential tests (the reference's `testing-mode` feature).
// Both carry the verifier's entries (host/tkmk_verify.hpp, host/tkmk_pairing.hpp): pure host work, no device call — except the device route
// of the two batch entries (host/tkmk_verify_device.hpp), which the caller asks for.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/tkmk_prover.h"
#include "tkmk_crs_audit.hpp"
#include "tkmk_crs_load.hpp"
#include "tkmk_service.hpp"
#include "tkmk_verify.hpp"
#include "tkmk_verify_device.hpp"

using namespace tkmk;

struct tkmk_prover {
    std::unique_ptr<ProverContext> ctx;
    std::mutex sigma2_mu;
    std::unique_ptr<verify::Sigma2> sigma2;   // the checked G2 side of the context's reference string (tkmk_prover_verify_batch), made on first use
};

static thread_local std::string g_last_error;
// libtkmk_hip.so takes calls from ONE host thread at a time per stream (include/tkmk.h "Threading"), and a prover context issues all its
// work on the default stream: two contexts of one process therefore take turns, whole calls at a time.  (The virtual ranks of a sharded
// prover over the loopback transport take turns through the communicator's device turn instead; RCCL ranks are one process per GPU.)
static std::mutex g_default_stream_mu;
struct DefaultStreamTurn {
    std::unique_lock<std::mutex> lk;
    explicit DefaultStreamTurn(bool sharded) : lk(g_default_stream_mu, std::defer_lock) {
        if (!sharded) lk.lock();
    }
};

template <class F>
static tkmk_error guarded(F &&fn) {
    try {
        fn();
        return TKMK_SUCCESS;
    } catch (const Error &e) {
        g_last_error = e.what();
        return e.code == TKMK_SUCCESS ? TKMK_ERR_UNKNOWN : e.code;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return TKMK_ERR_INVALID_ARGUMENT;
    } catch (...) {   // nothing foreign crosses the C ABI
        g_last_error = "unknown exception";
        return TKMK_ERR_UNKNOWN;
    }
}

#define TKP_API extern "C" __attribute__((visibility("default")))

TKP_API tkmk_error tkmk_prover_open(const char *subcircuit_library_dir, const char *crs_dir, tkmk_prover **out) {
    if (!subcircuit_library_dir || !crs_dir || !out) return TKMK_ERR_INVALID_POINTER;
    return guarded([&] {
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, "tkmk_prover_open: no HIP device (the MI355X backend has no CPU fallback)");
        std::string crs = crs_dir;
        DefaultStreamTurn turn(false);
        std::unique_ptr<tkmk_prover> p(new tkmk_prover());
        // TKMK_PROVER_CHECK_CRS=1: the audit of tkmk_crs_audit.hpp over the payload just loaded, before anything of it is uploaded for the
        // prover; a CRS that fails is refused and no context is made.  =2: with the table checks against the circuit of the library.
        // Unset or 0: nothing is added to what open does.
        CrsPayloadHook audit;
        if (crs_audit::requested_at_open())
            audit = [&](const CrsPayload &payload) {
                crs_audit::Report rep;
                const SetupParams sp = SetupParams::read(subcircuit_library_dir);
                if (!crs_audit::audit_payload(payload, sp, rep, crs_audit::circuit_requested_at_open(), subcircuit_library_dir)) throw Error("tkmk_prover_open: the reference string failed its audit (TKMK_PROVER_CHECK_CRS): " + rep.reason);
            };
        p->ctx = ProverContext::open(subcircuit_library_dir, crs, [&](const SetupParams &sp, std::string &source, const CrsGridHook &hook) { return load_prover_sigma(crs, sp, source, resident_table_c(sp), Shard{}, nullptr, hook, audit); });
        *out = p.release();
    });
}

static char *dup_string(const std::string &doc) {
    char *s = (char *)std::malloc(doc.size() + 1);
    if (!s) throw Error("out of memory");
    std::memcpy(s, doc.c_str(), doc.size() + 1);
    return s;
}

TKP_API tkmk_error tkmk_prover_open_sharded(void *comm, const char *subcircuit_library_dir, const char *crs_dir, tkmk_prover **out) {
    if (!comm || !subcircuit_library_dir || !crs_dir || !out) return TKMK_ERR_INVALID_POINTER;
    return guarded([&] {
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, "tkmk_prover_open_sharded: no HIP device (the MI355X backend has no CPU fallback)");
        ShardLink link = ShardLink::resolve(comm);   // the entries of libtkmk_dist.so, resolved at run time
        std::string crs = crs_dir;
        std::unique_ptr<tkmk_prover> p(new tkmk_prover());
        p->ctx = ProverContext::open(
            subcircuit_library_dir, crs, [&](const SetupParams &sp, std::string &source, const CrsGridHook &hook) { return load_prover_sigma(crs, sp, source, resident_table_c(sp, link.shard.world), link.shard, nullptr, hook); }, link);
        *out = p.release();
    });
}
TKP_API int tkmk_prover_world_size(const tkmk_prover *p) { return p && p->ctx->link ? (int)p->ctx->link.shard.world : 1; }

TKP_API tkmk_error tkmk_prover_prove(tkmk_prover *p, const char *synthesizer_dir, const char *output_dir, const char *testing_mixer_json,
                                     tkmk_prove_timing *timing, char **proof_json_out) {
    return tkmk_prover_prove_ex(p, synthesizer_dir, output_dir, testing_mixer_json, 0, timing, proof_json_out, nullptr);
}

TKP_API tkmk_error tkmk_prover_prove_ex(tkmk_prover *p, const char *synthesizer_dir, const char *output_dir, const char *testing_mixer_json, int flags,
                                        tkmk_prove_timing *timing, char **proof_json_out, char **commit_boxes_json_out) {
    if (!p || !synthesizer_dir) return TKMK_ERR_INVALID_POINTER;
    if (flags & ~(TKMK_PROVE_TEST_PARTS | TKMK_PROVE_COEFFICIENT_BASIS)) return TKMK_ERR_INVALID_ARGUMENT;
    if (proof_json_out) *proof_json_out = nullptr;
    if (commit_boxes_json_out) *commit_boxes_json_out = nullptr;
    std::vector<CommitBox> boxes;
    struct SinkGuard {   // the sink is thread-local and must not outlive `boxes`
        explicit SinkGuard(std::vector<CommitBox> *s) { commit_box_sink() = s; }
        ~SinkGuard() { commit_box_sink() = nullptr; }
    } sink_guard(commit_boxes_json_out ? &boxes : nullptr);
    return guarded([&] {
#ifdef TKMK_TESTING_MODE
        Mixer mixer = testing_mixer_json ? mixer_from_json(json::read_file(testing_mixer_json)) : Mixer::random();
#else
        // the reference gates fixed blinding scalars behind the compile-time feature `testing-mode`; so does this library
        if (testing_mixer_json) throw Error("tkmk_prover_prove: testing_mixer_json needs the testing-mode build (libtkmk_prover_testing.so); this library always draws its blinding scalars from getrandom()");
        Mixer mixer = Mixer::random();
#endif
        ProveTiming tm;
        DefaultStreamTurn turn((bool)p->ctx->link);
        Proof proof = p->ctx->prove(synthesizer_dir, output_dir ? output_dir : "", mixer, &tm, flags);
        if (timing) {
            timing->parse_s = tm.parse, timing->upload_s = tm.upload, timing->build_s = tm.build, timing->binding_s = tm.binding;
            timing->init_s = tm.init, timing->write_s = tm.write, timing->total_s = tm.total;
            for (int k = 0; k < 5; k++) timing->prove_s[k] = tm.prove[k];
        }
        if (proof_json_out) *proof_json_out = dup_string(proof.to_json());
        if (commit_boxes_json_out) {
            std::string doc = "[";
            for (size_t k = 0; k < boxes.size(); k++)
                doc += std::string(k ? ", " : "") + "{\"name\": \"" + boxes[k].name + "\", \"x\": " + std::to_string(boxes[k].x) + ", \"y\": " +
                       std::to_string(boxes[k].y) + ", \"basis\": \"" + boxes[k].basis + "\"}";
            *commit_boxes_json_out = dup_string(doc + "]");
        }
    });
}

TKP_API tkmk_error tkmk_prover_close(tkmk_prover *p) {
    if (!p) return TKMK_SUCCESS;
    return guarded([&] {
        DefaultStreamTurn turn((bool)p->ctx->link);
        delete p;
    });
}
TKP_API void tkmk_prover_free_string(char *s) { std::free(s); }
TKP_API const char *tkmk_prover_last_error(void) { return g_last_error.c_str(); }
TKP_API const char *tkmk_prover_crs_source(const tkmk_prover *p) { return p ? p->ctx->crs_source.c_str() : ""; }
TKP_API uint32_t tkmk_prover_root_generator(const tkmk_prover *p) { return p ? p->ctx->root_generator : 0; }

// ---- entries that answer with a verdict and, where asked for, a report document: both cleared first, then written by hand_over ----
template <class F>
static tkmk_error verdict_entry(int *ok, char **report_json_out, F &&fn) {
    *ok = 0;
    if (report_json_out) *report_json_out = nullptr;
    return guarded(fn);
}
template <class Report>
static void hand_over(bool verdict, const Report &rep, int *ok, char **report_json_out) {
    if (report_json_out) *report_json_out = dup_string(rep.to_json());
    *ok = verdict ? 1 : 0;
}

// ---- the verifier (host only: none of these touches the device, the default stream or a context's proving state) ----

TKP_API tkmk_error tkmk_pairing_product_is_one(const tkmk_g1_affine *p, const tkmk_g2_affine *q, size_t n, int *is_one) {
    if (!is_one || (n && (!p || !q))) return TKMK_ERR_INVALID_POINTER;
    *is_one = 0;
    return guarded([&] {
        std::vector<pairing::Pair> pairs(n);
        for (size_t i = 0; i < n; i++) {
            const char *why = pairing::g1_check(p[i], pairs[i].p);
            if (*why) throw Error("tkmk_pairing_product_is_one: G1 point " + std::to_string(i) + " " + why);
            why = pairing::g2_check(reinterpret_cast<const uint8_t *>(&q[i]), pairs[i].q);
            if (*why) throw Error("tkmk_pairing_product_is_one: G2 point " + std::to_string(i) + " " + why);
        }
        *is_one = pairing::product_is_one(pairs) ? 1 : 0;
    });
}

TKP_API tkmk_error tkmk_verify_files(const char *subcircuit_library_dir, const char *crs_dir, const char *synthesizer_dir, const char *preprocess_dir,
                                     const char *proof_dir, uint32_t root_generator, int *ok, char **report_json_out) {
    if (!subcircuit_library_dir || !crs_dir || !synthesizer_dir || !preprocess_dir || !proof_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        verify::Report rep;
        const bool verdict = verify::verify_files(subcircuit_library_dir, crs_dir, synthesizer_dir, preprocess_dir, proof_dir, root_generator, rep);
        hand_over(verdict, rep, ok, report_json_out);
    });
}

// the CRS audit (host/tkmk_crs_audit.hpp): device work on the default stream, so it takes the unsharded contexts' turn
static tkmk_error crs_audit_entry(const char *entry, const char *subcircuit_library_dir, const char *crs_dir, uint32_t flags, int *ok, char **report_json_out) {
    if (!subcircuit_library_dir || !crs_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        if (flags & ~(uint32_t)(TKMK_CRS_AUDIT_CIRCUIT | TKMK_CRS_AUDIT_LOCATE)) throw Error(TKMK_ERR_INVALID_ARGUMENT, std::string(entry) + ": unknown flag bits");
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, std::string(entry) + ": no HIP device (the MI355X backend has no CPU fallback)");
        DefaultStreamTurn turn(false);
        crs_audit::Report rep;
        const bool verdict = crs_audit::audit_files(subcircuit_library_dir, crs_dir, rep, nullptr, (flags & TKMK_CRS_AUDIT_CIRCUIT) != 0, (flags & TKMK_CRS_AUDIT_LOCATE) != 0);
        hand_over(verdict, rep, ok, report_json_out);
    });
}
// flags: TKMK_CRS_AUDIT_CIRCUIT = plus the gamma / eta / delta tables against the circuit of the library (audit_tables), TKMK_CRS_AUDIT_LOCATE =
// a failed structural check goes on to name the record
TKP_API tkmk_error tkmk_crs_audit_files_ex(const char *subcircuit_library_dir, const char *crs_dir, uint32_t flags, int *ok, char **report_json_out) {
    return crs_audit_entry("tkmk_crs_audit_files_ex", subcircuit_library_dir, crs_dir, flags, ok, report_json_out);
}
TKP_API tkmk_error tkmk_crs_audit_files(const char *subcircuit_library_dir, const char *crs_dir, int *ok, char **report_json_out) {
    return crs_audit_entry("tkmk_crs_audit_files", subcircuit_library_dir, crs_dir, 0, ok, report_json_out);
}
TKP_API tkmk_error tkmk_crs_audit_circuit_files(const char *subcircuit_library_dir, const char *crs_dir, int *ok, char **report_json_out) {
    return crs_audit_entry("tkmk_crs_audit_circuit_files", subcircuit_library_dir, crs_dir, TKMK_CRS_AUDIT_CIRCUIT, ok, report_json_out);
}

// the witness check (host/tkmk_witness_check.hpp; ProverContext::check_witness): device work on the default stream, like a proof
TKP_API tkmk_error tkmk_witness_check_files(const char *subcircuit_library_dir, const char *synthesizer_dir, int *ok, char **report_json_out) {
    if (!subcircuit_library_dir || !synthesizer_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, "tkmk_witness_check_files: no HIP device (the MI355X backend has no CPU fallback)");
        DefaultStreamTurn turn(false);
        std::unique_ptr<ProverContext> ctx = ProverContext::open_circuit(subcircuit_library_dir);   // no reference string
        witness_check::Report rep;
        const bool verdict = ctx->check_witness(synthesizer_dir, rep);
        hand_over(verdict, rep, ok, report_json_out);
    });
}
TKP_API tkmk_error tkmk_prover_check_witness(tkmk_prover *p, const char *synthesizer_dir, int *ok, char **report_json_out) {
    if (!p || !synthesizer_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        if (p->ctx->link)
            throw Error("tkmk_prover_check_witness: not available on a sharded context (the copy section crosses columns, and this entry is not collective: every rank calls tkmk_prover_check_witness_sharded instead)");
        DefaultStreamTurn turn(false);
        witness_check::Report rep;
        const bool verdict = p->ctx->check_witness(synthesizer_dir, rep);
        hand_over(verdict, rep, ok, report_json_out);
    });
}
// collective: every rank of a sharded context, with the same arguments (ProverContext::check_witness_sharded)
TKP_API tkmk_error tkmk_prover_check_witness_sharded(tkmk_prover *p, const char *synthesizer_dir, int *ok, char **report_json_out) {
    if (!p || !synthesizer_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        DefaultStreamTurn turn((bool)p->ctx->link);
        witness_check::Report rep;
        const bool verdict = p->ctx->check_witness_sharded(synthesizer_dir, rep);
        hand_over(verdict, rep, ok, report_json_out);
    });
}

TKP_API tkmk_error tkmk_prover_verify(tkmk_prover *p, const char *synthesizer_dir, const char *preprocess_dir, const char *proof_dir, int *ok,
                                      char **report_json_out) {
    if (!p || !synthesizer_dir || !preprocess_dir || !proof_dir || !ok) return TKMK_ERR_INVALID_POINTER;
    return verdict_entry(ok, report_json_out, [&] {
        const ProverContext &c = *p->ctx;
        verify::Inputs in;
        in.sp.n = c.sp.n, in.sp.l = c.sp.l, in.sp.l_D = c.sp.l_D, in.sp.s_max = c.sp.s_max, in.sp.l_user = c.sp.l_user, in.sp.l_free = c.sp.l_free;
        verify::validate_shape(in.sp);
        in.a_pub = verify::read_instance(synthesizer_dir, in.sp);
        verify::read_preprocess(preprocess_dir, in);
        verify::read_proof(proof_dir, in);
        // the reference string is the context's own: G, x, y, lagrange_KL of the G1Singles section and Sigma2 of the G2Points section
        const auto &s = c.sigma->g1_singles;
        in.pt[verify::CRS_G] = s[0], in.pt[verify::CRS_X] = s[1], in.pt[verify::CRS_Y] = s[2], in.pt[verify::CRS_KL] = s[5];
        for (int k = 0; k < verify::G2Count; k++) std::memcpy(in.g2[k].data(), c.sigma->g2_points.data() + 192 * k, 192);
        in.crs_label = c.crs_source;
        verify::Report rep;
        const bool verdict = verify::verify_loaded(in, c.root_generator, rep);   // the generator the context identified at open
        hand_over(verdict, rep, ok, report_json_out);
    });
}

// ---- batch verification (verify_batch of host/tkmk_verify.hpp; the device route is host/tkmk_verify_device.hpp) ----
// route HOST: pure host work, as the three entries above.  route DEVICE: upload, one tkmk_g1_check, per fold one tkmk_msm_segmented and / or one
// tkmk_msm_multi_ex call on the default stream, so it takes the unsharded contexts' turn, as the audit does.
static void batch_entry(const char *entry, const verify::Inputs &shared, const tkmk_verify_item *items, size_t n, uint32_t generator, int route,
                        std::unique_ptr<verify::Sigma2> *sigma2_cache, uint8_t *ok_each, int *ok_all, char **report_json_out) {
    if (n == 0) throw Error(std::string(entry) + ": an empty batch has no verdict (n must be at least 1)");
    if (route != TKMK_VERIFY_ROUTE_HOST && route != TKMK_VERIFY_ROUTE_DEVICE) throw Error(std::string(entry) + ": unknown route");
    std::vector<verify::BatchItem> list(n);
    for (size_t k = 0; k < n; k++) {
        if (!items[k].synthesizer_dir || !items[k].preprocess_dir || !items[k].proof_dir) throw Error(TKMK_ERR_INVALID_POINTER, std::string(entry) + ": item " + std::to_string(k));
        list[k] = {items[k].synthesizer_dir, items[k].preprocess_dir, items[k].proof_dir};
    }
    verify::BatchReport rep;
    if (route == TKMK_VERIFY_ROUTE_DEVICE) {
        int ndev = 0;
        if (tkmk_device_count(&ndev) != TKMK_SUCCESS || ndev < 1) throw Error(TKMK_ERR_NO_DEVICE, std::string(entry) + ": TKMK_VERIFY_ROUTE_DEVICE needs a HIP device (the host route does not)");
        DefaultStreamTurn turn(false);
        verify::DeviceFolder folder;
        verify::verify_batch(shared, list, generator, folder, rep, sigma2_cache);
    } else {
        verify::HostFolder folder;
        verify::verify_batch(shared, list, generator, folder, rep, sigma2_cache);
    }
    for (size_t k = 0; k < n; k++) ok_each[k] = rep.items[k].ok ? 1 : 0;
    if (report_json_out) *report_json_out = dup_string(rep.to_json());
    *ok_all = rep.ok ? 1 : 0;
}

TKP_API tkmk_error tkmk_verify_batch_files(const char *subcircuit_library_dir, const char *crs_dir, const tkmk_verify_item *items, size_t n, uint32_t root_generator,
                                           int route, uint8_t *ok_each, int *ok_all, char **report_json_out) {
    if (!subcircuit_library_dir || !crs_dir || !ok_all || (n && (!items || !ok_each))) return TKMK_ERR_INVALID_POINTER;
    *ok_all = 0;
    if (n) std::memset(ok_each, 0, n);
    if (report_json_out) *report_json_out = nullptr;
    return guarded([&] {
        if (n == 0) throw Error("tkmk_verify_batch_files: an empty batch has no verdict (n must be at least 1)");
        verify::Inputs shared;
        shared.sp = verify::read_shape(subcircuit_library_dir);
        verify::validate_shape(shared.sp);
        verify::read_sigma_verify(crs_dir, shared);
        batch_entry("tkmk_verify_batch_files", shared, items, n, root_generator, route, nullptr, ok_each, ok_all, report_json_out);
    });
}

TKP_API tkmk_error tkmk_prover_verify_batch(tkmk_prover *p, const tkmk_verify_item *items, size_t n, int route, uint8_t *ok_each, int *ok_all, char **report_json_out) {
    if (!p || !ok_all || (n && (!items || !ok_each))) return TKMK_ERR_INVALID_POINTER;
    *ok_all = 0;
    if (n) std::memset(ok_each, 0, n);
    if (report_json_out) *report_json_out = nullptr;
    return guarded([&] {
        const ProverContext &c = *p->ctx;
        if (route == TKMK_VERIFY_ROUTE_DEVICE && c.link)
            throw Error("tkmk_prover_verify_batch: TKMK_VERIFY_ROUTE_DEVICE is not available on a sharded context (its ranks keep the host route, which needs no collective)");
        verify::Inputs shared;
        shared.sp.n = c.sp.n, shared.sp.l = c.sp.l, shared.sp.l_D = c.sp.l_D, shared.sp.s_max = c.sp.s_max, shared.sp.l_user = c.sp.l_user, shared.sp.l_free = c.sp.l_free;
        const auto &s = c.sigma->g1_singles;
        shared.pt[verify::CRS_G] = s[0], shared.pt[verify::CRS_X] = s[1], shared.pt[verify::CRS_Y] = s[2], shared.pt[verify::CRS_KL] = s[5];
        for (int k = 0; k < verify::G2Count; k++) std::memcpy(shared.g2[k].data(), c.sigma->g2_points.data() + 192 * k, 192);
        shared.crs_label = c.crs_source;
        std::lock_guard<std::mutex> lk(p->sigma2_mu);   // the Sigma2 check of this context's reference string: once per context
        batch_entry("tkmk_prover_verify_batch", shared, items, n, c.root_generator, route, &p->sigma2, ok_each, ok_all, report_json_out);
    });
}
