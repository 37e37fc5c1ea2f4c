// crsaudit.hip — the two small kernels the circuit part of the CRS audit needs beside the MSM and the bivariate NTT
// (host/tkmk_crs_audit.hpp audit_tables: the gamma / eta / delta tables against the circuit polynomials).
//
//   tkmk_fr_outer           out[j * out_stride + i] = col[j] * row[i]: the rank-one grids a_j b_i the audit combines a table with, and
//                           the evaluation grids (A a)[c] b_i.  One lane per output element; nothing is staged on the host (the
//                           setup's outer_scaled builds the same product from two host index arrays and two gathers).
//   tkmk_r1cs_library_mix   weights per WIRE instead of values per placement: u[c][g] = sum over kinds, over the entries of row c of
//                           A_kind whose wire routes to column g, of coeff * weight[kind][wire]; v, w from B, C.  One lane per
//                           (constraint row, matrix) walks every kind in order, so the sum over kinds is deterministic and needs no
//                           atomics; every element of [0, n) x [0, n_cols) is written, zeros included.
// Neither is a hot path: both are bound by the reads of their operands and run a handful of times per audit.
#include "common.h"
#include "r1cs_library.h"

__global__ __launch_bounds__(256) void k_fr_outer(const fr_t *__restrict__ col, const fr_t *__restrict__ row, uint64_t total, uint32_t cols,
                                                 uint32_t out_stride, fr_t *__restrict__ out) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    uint32_t j = (uint32_t)(e / cols), i = (uint32_t)(e - (uint64_t)j * cols);
    fr_t r = Fr::mul(Fr::to_mont(Fr::canon(tk_load(col + j))), Fr::canon(tk_load(row + i)));   // Montgomery * plain -> plain
    tk_store(out + (uint64_t)j * out_stride + i, r);
}

TK_API tkmk_error tkmk_fr_outer(const tkmk_fr *col_dev, uint32_t rows, const tkmk_fr *row_dev, uint32_t cols, uint32_t out_stride, tkmk_fr *out_dev,
                                tkmk_stream stream) {
    if (rows == 0 || cols == 0) return TKMK_SUCCESS;
    if (!col_dev || !row_dev || !out_dev) return TKMK_ERR_INVALID_POINTER;
    if (out_stride < cols) return TKMK_ERR_INVALID_ARGUMENT;
    const uint64_t total = (uint64_t)rows * cols;
    if (total >= (1ull << 40)) return TKMK_ERR_INVALID_ARGUMENT;   // the grid stays below 2^32 blocks
    TK_TRY(tk_require_device());
    hipStream_t s = tk_stream(stream);
    hipLaunchKernelGGL(k_fr_outer, tk_div_up(total, 256), 256, 0, s, (const fr_t *)col_dev, (const fr_t *)row_dev, total, cols, out_stride, (fr_t *)out_dev);
    TK_HIP(hipGetLastError());
    return TKMK_SUCCESS;
}

// desc as in witness.hip (8 u32 per kind: rowptr base of A, B, C; entry base of A, B, C; n_rows; n_wires).  weight[kind]: n_wires plain Fr;
// col: NULL, or per kind NULL (every wire of it routes to column 0) or n_wires bytes, each < n_cols (checked by the launcher).
__global__ __launch_bounds__(256) void k_r1cs_library_mix(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ wire,
                                                         const fr_t *__restrict__ coeff_mont, const uint32_t *__restrict__ desc, uint32_t n_sub,
                                                         const fr_t *const *__restrict__ weight, const uint8_t *const *__restrict__ col, uint32_t n,
                                                         uint32_t n_cols, uint32_t out_stride, fr_t *__restrict__ u, fr_t *__restrict__ v,
                                                         fr_t *__restrict__ w) {
    const uint32_t m = blockIdx.y;
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    fr_t *out = (m == 0 ? u : m == 1 ? v : w) + (uint64_t)row * out_stride;
    for (uint32_t g = 0; g < n_cols; g++) {
        fr_t acc = Fr::zero();
        for (uint32_t s = 0; s < n_sub; s++) {
            const uint32_t *d = desc + 8 * s;
            if (row >= d[6]) continue;   // rows past a kind's constraint count contribute nothing
            const uint32_t *rp = rowptr + d[m];
            const uint32_t eb = d[3 + m];
            const fr_t *wt = weight[s];
            const uint8_t *cl = col ? col[s] : nullptr;
            for (uint32_t k = rp[row]; k < rp[row + 1]; k++) {
                const uint32_t wi = wire[eb + k];
                if ((cl ? (uint32_t)cl[wi] : 0u) != g) continue;
                acc = Fr::add(acc, Fr::mul(Fr::canon(tk_load(wt + wi)), tk_load(coeff_mont + eb + k)));   // plain * Montgomery -> plain
            }
        }
        tk_store(out + g, acc);
    }
}

TK_API tkmk_error tkmk_r1cs_library_mix(const tkmk_r1cs_library *lib, const tkmk_fr *const *weight_dev, const uint8_t *const *col_dev, uint32_t n,
                                        uint32_t n_cols, uint32_t out_stride, tkmk_fr *u_dev, tkmk_fr *v_dev, tkmk_fr *w_dev, tkmk_stream stream) {
    if (!lib || !u_dev || !v_dev || !w_dev) return TKMK_ERR_INVALID_POINTER;
    if (lib->n_sub && !weight_dev) return TKMK_ERR_INVALID_POINTER;
    if (n_cols == 0 || n_cols > out_stride || n_cols > 255 || lib->max_rows > n) return TKMK_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < lib->n_sub; k++)
        if (!weight_dev[k] && lib->n_wires[k]) return TKMK_ERR_INVALID_POINTER;
    if (n == 0) return TKMK_SUCCESS;
    TK_TRY(tk_require_device());
    hipStream_t s = tk_stream(stream);
    // the routing bytes decide which output column a lane writes: checked here, once per call, so that the kernel cannot be sent
    // outside [0, n_cols)
    if (col_dev) {
        std::vector<uint8_t> h;
        TK_HIP(hipStreamSynchronize(s));   // whatever filled the arrays on this stream has finished
        for (uint32_t k = 0; k < lib->n_sub; k++) {
            if (!col_dev[k] || !lib->n_wires[k]) continue;
            h.resize(lib->n_wires[k]);
            TK_HIP(hipMemcpy(h.data(), col_dev[k], h.size(), hipMemcpyDeviceToHost));
            for (uint8_t c : h)
                if (c >= n_cols) return TKMK_ERR_INVALID_ARGUMENT;
        }
    }
    tk_frame frame(s);
    const size_t pb = (size_t)(lib->n_sub ? lib->n_sub : 1) * sizeof(void *);
    tk_scratch d_weight, d_col;
    TK_TRY(d_weight.alloc(pb, s));
    if (lib->n_sub) TK_HIP(hipMemcpyAsync(d_weight.p, weight_dev, (size_t)lib->n_sub * sizeof(void *), hipMemcpyHostToDevice, s));
    if (col_dev) {
        TK_TRY(d_col.alloc(pb, s));
        if (lib->n_sub) TK_HIP(hipMemcpyAsync(d_col.p, col_dev, (size_t)lib->n_sub * sizeof(void *), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_r1cs_library_mix, dim3(tk_div_up(n, 256), 3, 1), 256, 0, s, lib->d_rowptr, lib->d_wire, (const fr_t *)lib->d_coeff, lib->d_desc,
                       lib->n_sub, (const fr_t *const *)d_weight.p, (const uint8_t *const *)d_col.p, n, n_cols, out_stride, (fr_t *)u_dev, (fr_t *)v_dev,
                       (fr_t *)w_dev);
    TK_HIP(hipGetLastError());
    // the pointer tables above were copied from the caller's host arrays and live in this call's frame: the call returns when the
    // kernel has read them
    TK_HIP(hipStreamSynchronize(s));
    return TKMK_SUCCESS;
}
