// tkmk_verify_device.hpp — the device route of verify_batch (host/tkmk_verify.hpp): a Folder and a membership pass over libtkmk_hip.so.
// Compiled into libtkmk_prover.so only; bin/verify keeps the host route and links neither the device library nor the ROCm runtime.
// The fold of a batch IS ten multi-scalar multiplications over the batch's distinct G1 records, and its membership pass IS the batched
// check the CRS audit runs, so the route is
//   upload      the distinct records, plain affine, once per batch (kept for the re-folds of a bisection);
//   membership  ONE tkmk_g1_check call with a verdict byte per record (csrc/g1check.hip: the first of not reduced / off the curve / outside
//               the subgroup; the all-zero record is infinity and passes, as on the host);
//   fold        the ten slot jobs address the uploaded table through base_index lists (base_table_len set, so an index is checked on the
//               device and never read out of bounds).  The jobs of at most kSegmentedMaxTerms terms — six of the ten have ONE term at every
//               batch size — go into ONE tkmk_msm_segmented call (two launches, the tail on the device), the rest into ONE
//               tkmk_msm_multi_ex call (plain windows, no precomputed table); either call may be absent; ten projective results come back;
//   pairing     on the host (verify_batch).
// Everything runs on the default stream under the caller's DefaultStreamTurn (host/prover_abi.cpp), in buffers this object allocates and
// frees.  It reads and changes no library or context state: no NTT domain, no root-of-unity generator, no commit table — the MSM and the
// membership kernel are stateless apart from the library's scratch arenas.  Not for a sharded context: its ranks keep the host route,
// which needs no collective.
#pragma once
#include "tkmk_host.hpp"
#include "tkmk_protocol.hpp"
#include "tkmk_verify.hpp"

namespace tkmk {
namespace verify {

// A slot job of at most this many terms goes to tkmk_msm_segmented, a longer one to the sorting pipeline.  From the crossover measured by
// tools/msm_segmented_bench.py on ten equal jobs (profiles/msm_segmented.json): 2.7 ms against 4.8 ms at 1024 terms,
// 4.4 against 4.6 at 2048, 7.8 against 4.8 at 4096.  The crossover is 2048, by a margin inside the spread of a shared box; a fold's jobs are
// unequal and its longest job sets the segmented kernel's time — so the constant is the last size with a clear margin, and the batch
// figures of section 8 were taken with it.
constexpr size_t kSegmentedMaxTerms = 1024;
static_assert(kSegmentedMaxTerms <= TKMK_MSM_SEGMENTED_MAX_SIZE, "the segmented entry refuses longer jobs");

struct DeviceFolder : Folder {
    DeviceVec<G1Affine> table;            // the batch's distinct records
    const tkmk_g1_affine *table_of = nullptr;   // the host vector `table` was uploaded from
    const char *route() const override { return "device"; }
    void upload(const std::vector<tkmk_g1_affine> &records) {
        if (table_of == records.data() && table.len() == records.size()) return;
        if (records.size() >= (1ull << 31)) throw Error("verify_batch: too many records for one device table");
        table = DeviceVec<G1Affine>::from_host(records);
        table_of = records.data();
    }
    void membership(const std::vector<tkmk_g1_affine> &records, std::vector<uint8_t> &verdict) override {
        verdict.assign(records.size(), 0);
        if (records.empty()) return;
        upload(records);
        DeviceVec<uint8_t> v(records.size());
        tkmk_g1_check_report r{};
        check(tkmk_g1_check(table.ptr(), TKMK_BASES_PLAIN, records.size(), 0, 0, v.ptr(), &r, nullptr), "tkmk_g1_check");
        v.copy_to_host(verdict.data(), verdict.size());
    }
    void fold(const std::vector<tkmk_g1_affine> &records, const std::vector<FoldTerm> (&slot)[kSlots], tkmk_g1_affine (&out)[kSlots]) override {
        upload(records);
        size_t total = 0, off[kSlots + 1] = {0};
        for (int j = 0; j < kSlots; j++) off[j + 1] = total += slot[j].size();
        for (tkmk_g1_affine &o : out) o = tkmk_g1_affine{};
        if (total == 0) return;
        std::vector<ScalarField> scalars(total);
        std::vector<uint32_t> index(total);
        for (int j = 0; j < kSlots; j++)
            for (size_t t = 0; t < slot[j].size(); t++) {
                if (slot[j][t].record >= records.size()) throw Error("verify_batch: a fold term names a record outside the table");
                scalars[off[j] + t] = slot[j][t].scalar, index[off[j] + t] = slot[j][t].record;
            }
        DeviceVec<ScalarField> d_scalars = DeviceVec<ScalarField>::from_host(scalars);
        DeviceVec<uint32_t> d_index = DeviceVec<uint32_t>::from_host(index);
        // jobs[0, n_small): the slots of at most kSegmentedMaxTerms terms, in slot order; jobs[kSlots - n_large, kSlots): the rest
        tkmk_msm_job_ex jobs[kSlots] = {};
        int at[kSlots], n_small = 0, n_large = 0;
        for (int j = 0; j < kSlots; j++) at[j] = slot[j].size() <= kSegmentedMaxTerms ? n_small++ : kSlots - 1 - n_large++;
        for (int j = 0; j < kSlots; j++) {
            tkmk_msm_job_ex &job = jobs[at[j]];
            job.scalars = d_scalars.ptr() + off[j], job.bases = table.ptr(), job.msm_size = (int)slot[j].size();
            job.base_index = d_index.ptr() + off[j], job.base_table_len = table.len();
        }
        tkmk_msm_config cfg = tkmk_msm_default_config();
        cfg.are_scalars_on_device = cfg.are_points_on_device = true;
        tkmk_g1_projective sums[kSlots];
        if (n_small) check(tkmk_msm_segmented(jobs, n_small, &cfg, TKMK_BASES_PLAIN, sums), "tkmk_msm_segmented");
        if (n_large) check(tkmk_msm_multi_ex(jobs + n_small, n_large, &cfg, TKMK_BASES_PLAIN, sums + n_small), "tkmk_msm_multi_ex");
        segmented_jobs += (uint64_t)n_small, pipeline_jobs += (uint64_t)n_large;
        for (int j = 0; j < kSlots; j++) out[j] = projective_to_affine(sums[at[j]]);
    }
};

}  // namespace verify
}  // namespace tkmk
