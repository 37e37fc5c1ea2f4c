// crs_identify.hip — which two-adic root of unity a reference string was made under (tkmk_crs_identify_root, include/tkmk.h).
//
// The CRS carries lagrange_KL = [L_{s_max-1}(tau_y) K_{m_I-1}(tau_x)] G (libs/src/group_structures/mod.rs:326-327) next to the monomial
// table xy_powers[a * rs_y + b] = [tau_x^a tau_y^b] G.  The last Lagrange polynomial of the n-th roots of unity is
// L_{n-1}(X) = (1 / n) sum_j w_n^j X^j (w^{-j (n-1)} = w^j), hence
//     lagrange_KL = sum_{a < m_I} sum_{b < s_max} (w_x^a / m_I) (w_y^b / s_max) xy_powers[a * rs_y + b]:
// one MSM over the m_I x s_max corner of the table with a rank-one geometric scalar grid that depends on the generator the roots derive
// from.  One grid (tkmk_poly_geometric_grid) and one job of a tkmk_msm_multi_ex batch per candidate, all over the same view of the bases;
// plain windows, no precomputed table: the check runs before a context has built one, on the records as they are at that moment.
#include "common.h"

// idx[a * lc + k] = a * rs_y + col0 + col_step * k: the strided-column view of the corner as a base_index list
__global__ __launch_bounds__(256) void k_corner_index(uint32_t *__restrict__ idx, uint32_t m_i, uint32_t lc, uint32_t rs_y, uint32_t col0, uint32_t col_step) {
    const uint64_t total = (uint64_t)m_i * lc;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = (uint32_t)(e / lc), k = (uint32_t)(e - (uint64_t)a * lc);
        idx[e] = a * rs_y + col0 + col_step * k;   // < h_max * rs_y < 2^31 (checked by the launcher)
    }
}

namespace {
struct dev_buf {   // the library's caching allocator: freed blocks are reused only after the work queued before the free has finished
    void *p = nullptr;
    ~dev_buf() {
        if (p) (void)tkmk_free(p);
    }
};
}  // namespace

TK_API tkmk_error tkmk_crs_identify_root(const tkmk_g1_affine *xy_powers_dev, int bases_form, uint32_t h_max, uint32_t rs_y, uint32_t m_i, uint32_t s_max,
                                         uint32_t col0, uint32_t col_step, const uint32_t *candidates, int n_candidates, tkmk_g1_projective *partial_out) {
    if (!xy_powers_dev || !candidates || !partial_out) return TKMK_ERR_INVALID_POINTER;
    if (bases_form != TKMK_BASES_PLAIN && bases_form != TKMK_BASES_MONTGOMERY && bases_form != TKMK_BASES_CONVERTED) return TKMK_ERR_INVALID_ARGUMENT;
    if (n_candidates < 1 || n_candidates > 8 || !col_step) return TKMK_ERR_INVALID_ARGUMENT;
    if (tk_log2_exact(m_i) < 0 || tk_log2_exact(s_max) < 0 || m_i > h_max || s_max > rs_y) return TKMK_ERR_INVALID_ARGUMENT;
    if ((uint64_t)h_max * rs_y >= (1ull << 31) || (uint64_t)m_i * s_max >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
    TK_TRY(tk_require_device());
    const uint32_t lc = col0 < s_max ? (s_max - col0 + col_step - 1) / col_step : 0;   // |{k : col0 + col_step k < s_max}|
    const uint64_t size = (uint64_t)m_i * lc;

    // 1 / (m_I s_max), plain
    fr_t c0;
    {
        fr_t a = Fr::zero(), b = Fr::zero();
        a.l[0] = m_i, b.l[0] = s_max;
        c0 = Fr::from_mont(Fr::inv(Fr::mul(Fr::to_mont(a), Fr::to_mont(b))));
    }
    tkmk_fr c0_api;
    for (int i = 0; i < 8; i++) c0_api.limbs[i] = c0.l[i];

    dev_buf scalars, index;
    std::vector<tkmk_msm_job_ex> jobs((size_t)n_candidates);
    if (size) {
        TK_TRY(tkmk_malloc(&scalars.p, (size_t)n_candidates * size * sizeof(tkmk_fr)));
        if (col_step != 1) {
            TK_TRY(tkmk_malloc(&index.p, size * sizeof(uint32_t)));
            uint64_t g = (size + 255) / 256;
            hipLaunchKernelGGL(k_corner_index, (unsigned)(g > 4096 ? 4096 : g), 256, 0, nullptr, (uint32_t *)index.p, m_i, lc, rs_y, col0, col_step);
            TK_HIP(hipGetLastError());
        }
    }
    for (int c = 0; c < n_candidates; c++) {
        tkmk_fr wx, wy;
        // a residue (or a generator < 2) among the candidates is the caller's mistake: TKMK_ERR_INVALID_ARGUMENT, as get_root_of_unity gives
        TK_TRY(bls12_381_get_root_of_unity_with_generator(candidates[c], m_i, &wx));
        TK_TRY(bls12_381_get_root_of_unity_with_generator(candidates[c], s_max, &wy));
        tkmk_msm_job_ex j{};
        j.msm_size = (int)size;
        if (size) {
            tkmk_fr *grid = (tkmk_fr *)scalars.p + (size_t)c * size;
            TK_TRY(tkmk_poly_geometric_grid(m_i, lc, &c0_api, &wx, &wy, col0, col_step, grid, nullptr));
            j.scalars = grid;
            if (col_step == 1) {   // contiguous columns [col0, col0 + lc) of every row: a strided view
                j.bases = xy_powers_dev + col0;
                j.base_cols = lc, j.base_stride = rs_y;
                j.base_table_len = (uint64_t)h_max * rs_y - col0;
            } else {
                j.bases = xy_powers_dev;
                j.base_index = (const uint32_t *)index.p;
                j.base_table_len = (uint64_t)h_max * rs_y;
            }
        }
        jobs[(size_t)c] = j;
    }
    tkmk_msm_config cfg = tkmk_msm_default_config();
    cfg.are_scalars_on_device = cfg.are_points_on_device = true;
    return tkmk_msm_multi_ex(jobs.data(), n_candidates, &cfg, bases_form, partial_out);
}
