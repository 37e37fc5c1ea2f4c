// witcheck.hip — the witness check on the device (host/tkmk_witness_check.hpp): two streaming passes over grids Prover::init has
// already built.  The reference has the same two diagnostics behind its `testing-mode` feature, as host loops over downloaded evaluations
// (prove/src/lib.rs:916-1017 the copy flags, 1472-1518 "Placement indexed at {} does not satisfy R1CS").
//
//   tkmk_witness_check_r1cs   u . v = w cell by cell over three rows x stride evaluation grids (the layout tkmk_r1cs_library_eval writes):
//                             per column the count of failing rows and the smallest failing row
//   tkmk_witness_check_copy   b[dst[e]] = b[X[e] * stride + Y[e]] entry by entry over the de-duplicated permutation arrays
//   tkmk_witness_check_copy_split   the same comparison on one rank of a sharded prover: b_local[dst[e]] = sources[slot[e]]
//
// Both results are a count and a minimum over integers: they do not depend on the order the workgroups arrive in.  The field product is
// Fr::mul of ff.h.
#include "common.h"

// One lane per cell, the column index fastest: a wave reads 64 consecutive columns of one row (32-byte elements, 2 KB contiguous), the four
// waves of a workgroup take four consecutive rows and walk down a chunk of rows_per_block rows, four at a time.  A lane keeps its column's
// count and first failing row in registers over the walk; the four waves meet in LDS, and a column that saw a failure costs the workgroup
// one atomicAdd and one atomicMin — a grid in which every cell fails issues rows / rows_per_block of them per column, not one per cell.
__global__ __launch_bounds__(256) void k_witness_check_r1cs(const fr_t *__restrict__ u, const fr_t *__restrict__ v, const fr_t *__restrict__ w,
                                                           uint32_t n_rows, uint32_t n_cols, uint32_t stride, uint32_t rows_per_block,
                                                           uint32_t *__restrict__ bad_count, uint32_t *__restrict__ first_bad_row) {
    __shared__ uint32_t s_cnt[4][64], s_min[4][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t col = blockIdx.x * 64u + lane;
    const uint64_t row0 = (uint64_t)blockIdx.y * rows_per_block;
    const uint64_t row_end = row0 + rows_per_block < n_rows ? row0 + rows_per_block : n_rows;
    uint32_t cnt = 0, first = 0xFFFFFFFFu;
    if (col < n_cols)   // the padding columns [n_cols, stride) are never read
        for (uint64_t row = row0 + wave; row < row_end; row += 4) {
            const uint64_t at = row * stride + col;
            const fr_t a = Fr::canon(tk_load(u + at)), b = Fr::canon(tk_load(v + at)), c = Fr::canon(tk_load(w + at));
            if (!Fr::eq(Fr::mul(Fr::to_mont(a), b), c)) {   // Montgomery * plain -> plain
                cnt++;
                if (first == 0xFFFFFFFFu) first = (uint32_t)row;   // rows ascend along the walk
            }
        }
    s_cnt[wave][lane] = cnt, s_min[wave][lane] = first;
    __syncthreads();
    if (wave == 0 && col < n_cols) {
        for (int k = 1; k < 4; k++) {
            cnt += s_cnt[k][lane];
            first = s_min[k][lane] < first ? s_min[k][lane] : first;
        }
        if (cnt) {
            atomicAdd(bad_count + col, cnt);
            atomicMin(first_bad_row + col, first);
        }
    }
}

TK_API tkmk_error tkmk_witness_check_r1cs(const tkmk_fr *u_dev, const tkmk_fr *v_dev, const tkmk_fr *w_dev, uint32_t n_rows, uint32_t n_cols,
                                          uint32_t stride, uint32_t *bad_count_dev, uint32_t *first_bad_row_dev, uint64_t *total_bad_out,
                                          tkmk_stream stream) {
    if (!total_bad_out) return TKMK_ERR_INVALID_POINTER;
    *total_bad_out = 0;
    if (n_cols > stride) return TKMK_ERR_INVALID_ARGUMENT;
    if (n_cols == 0) return TKMK_SUCCESS;
    if (!bad_count_dev || !first_bad_row_dev) return TKMK_ERR_INVALID_POINTER;
    if (n_rows && (!u_dev || !v_dev || !w_dev)) return TKMK_ERR_INVALID_POINTER;
    if (n_rows == 0xFFFFFFFFu) return TKMK_ERR_INVALID_ARGUMENT;   // a row index is reported in 32 bits and 0xFFFFFFFF means "none"
    TK_TRY(tk_require_device());
    hipStream_t s = tk_stream(stream);
    TK_HIP(hipMemsetAsync(bad_count_dev, 0, (size_t)n_cols * 4, s));
    TK_HIP(hipMemsetAsync(first_bad_row_dev, 0xFF, (size_t)n_cols * 4, s));
    if (n_rows) {
        // chunks of 64 rows; more where the grid's y dimension (65535) would not hold them
        uint32_t rows_per_block = 64;
        while (tk_div_up(n_rows, rows_per_block) > 65535u) rows_per_block *= 2;
        hipLaunchKernelGGL(k_witness_check_r1cs, dim3(tk_div_up(n_cols, 64), tk_div_up(n_rows, rows_per_block)), 256, 0, s, (const fr_t *)u_dev,
                           (const fr_t *)v_dev, (const fr_t *)w_dev, n_rows, n_cols, stride, rows_per_block, bad_count_dev, first_bad_row_dev);
        TK_HIP(hipGetLastError());
    }
    std::vector<uint32_t> counts(n_cols);
    TK_HIP(hipMemcpyAsync(counts.data(), bad_count_dev, (size_t)n_cols * 4, hipMemcpyDeviceToHost, s));
    TK_HIP(hipStreamSynchronize(s));
    uint64_t total = 0;
    for (uint32_t c : counts) total += c;
    *total_bad_out = total;
    return TKMK_SUCCESS;
}

// The copy comparison, one lane per entry.  WHICH two cells entry e compares is its caller's addressing (a functor: false when the entry
// points outside its buffers — such an entry is never dereferenced, is counted in res[2] and takes no part in the verdict); everything
// else is shared.  A wave's failing lanes are a ballot: their number is its population count and the first of them its lowest set bit
// (lane order is entry order); the four waves of a workgroup meet in LDS and a workgroup that saw a failure issues one atomicAdd and one
// atomicMin.   res: [0] bad entries, [1] first bad entry, [2] invalid entries
template <class Cells>
__global__ __launch_bounds__(256) void k_witness_check_copy(const Cells cells, uint64_t n, unsigned long long *__restrict__ res) {
    __shared__ unsigned long long s_bad[4], s_first[4], s_inv[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, invalid = false;
    if (e < n) {
        const fr_t *value, *source;
        if (!cells(e, value, source)) invalid = true;
        else bad = !Fr::eq(Fr::canon(tk_load(value)), Fr::canon(tk_load(source)));
    }
    const unsigned long long m_bad = __ballot(bad), m_inv = __ballot(invalid);
    if (lane == 0) {
        s_bad[wave] = (unsigned long long)__popcll(m_bad);
        s_first[wave] = m_bad ? e + (unsigned long long)(__ffsll((long long)m_bad) - 1) : ~0ull;
        s_inv[wave] = (unsigned long long)__popcll(m_inv);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long nb = 0, ni = 0, first = ~0ull;
        for (int k = 0; k < 4; k++) nb += s_bad[k], ni += s_inv[k], first = s_first[k] < first ? s_first[k] : first;
        if (nb) atomicAdd(res + 0, nb), atomicMin(res + 1, first);
        if (ni) atomicAdd(res + 2, ni);
    }
}

// b[dst[e]] against b[X[e] * stride + Y[e]] inside the rows x cols cells of one stride-wide grid
struct CopyCellsGrid {
    const fr_t *b;
    uint32_t rows, cols, stride;
    const uint32_t *dst_idx, *src_x, *src_y;
    __device__ bool operator()(uint64_t e, const fr_t *&value, const fr_t *&source) const {
        const uint32_t d = dst_idx[e], x = src_x[e], y = src_y[e];
        if (d / stride >= rows || d % stride >= cols || x >= rows || y >= cols) return false;
        value = b + d, source = b + (uint64_t)x * stride + y;
        return true;
    }
};
// One rank of a sharded prover: the destination cells are this rank's own (b_local, its columns of b), the source values arrive packed
// from every rank in one gathered buffer (the copy section of host/tkmk_witness_check.hpp).  One 32-byte load from each buffer: the
// destination indices ascend, the slots mostly do.
struct CopyCellsSplit {
    const fr_t *b_local, *sources;
    uint64_t local_cells, n_sources;
    const uint32_t *dst_local, *src_slot;
    __device__ bool operator()(uint64_t e, const fr_t *&value, const fr_t *&source) const {
        const uint32_t d = dst_local[e], s = src_slot[e];
        if (d >= local_cells || s >= n_sources) return false;
        value = b_local + d, source = sources + s;
        return true;
    }
};

// what both entries do once their arguments are checked: one workgroup per 256 entries, three counters down and up
template <class Cells>
static tkmk_error witness_check_copy_run(const Cells &cells, uint64_t n, uint64_t *bad_entries_out, uint64_t *first_bad_entry_out, tkmk_stream stream) {
    TK_TRY(tk_require_device());
    hipStream_t s = tk_stream(stream);
    tk_frame frame(s);
    tk_scratch d_res;
    TK_TRY(d_res.alloc(3 * sizeof(unsigned long long), s));
    const unsigned long long init[3] = {0ull, ~0ull, 0ull};
    TK_HIP(hipMemcpyAsync(d_res.p, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_witness_check_copy<Cells>, tk_div_up(n, 256), 256, 0, s, cells, n, d_res.as<unsigned long long>());
    TK_HIP(hipGetLastError());
    unsigned long long res[3] = {0, 0, 0};
    TK_HIP(hipMemcpyAsync(res, d_res.p, sizeof res, hipMemcpyDeviceToHost, s));
    TK_HIP(hipStreamSynchronize(s));
    *bad_entries_out = res[0], *first_bad_entry_out = res[1];
    return res[2] ? TKMK_ERR_INVALID_ARGUMENT : TKMK_SUCCESS;
}

TK_API tkmk_error tkmk_witness_check_copy(const tkmk_fr *b_dev, uint32_t rows, uint32_t cols, uint32_t stride, const uint32_t *dst_idx_dev,
                                          const uint32_t *src_x_dev, const uint32_t *src_y_dev, uint64_t n_entries, uint64_t *bad_entries_out,
                                          uint64_t *first_bad_entry_out, tkmk_stream stream) {
    if (!bad_entries_out || !first_bad_entry_out) return TKMK_ERR_INVALID_POINTER;
    *bad_entries_out = 0, *first_bad_entry_out = UINT64_MAX;
    if (cols > stride) return TKMK_ERR_INVALID_ARGUMENT;
    if (n_entries == 0) return TKMK_SUCCESS;
    if (!b_dev || !dst_idx_dev || !src_x_dev || !src_y_dev) return TKMK_ERR_INVALID_POINTER;
    if (stride == 0 || n_entries > (0x7FFFFFFFull << 8)) return TKMK_ERR_INVALID_ARGUMENT;   // one workgroup per 256 entries
    return witness_check_copy_run(CopyCellsGrid{(const fr_t *)b_dev, rows, cols, stride, dst_idx_dev, src_x_dev, src_y_dev}, n_entries, bad_entries_out,
                                  first_bad_entry_out, stream);
}

TK_API tkmk_error tkmk_witness_check_copy_split(const tkmk_fr *b_local_dev, uint64_t local_cells, const uint32_t *dst_local_dev,
                                                const tkmk_fr *sources_dev, uint64_t n_sources, const uint32_t *src_slot_dev, uint64_t n,
                                                uint64_t *bad_entries_out, uint64_t *first_bad_entry_out, tkmk_stream stream) {
    if (!bad_entries_out || !first_bad_entry_out) return TKMK_ERR_INVALID_POINTER;
    *bad_entries_out = 0, *first_bad_entry_out = UINT64_MAX;
    if (n == 0) return TKMK_SUCCESS;
    if (!b_local_dev || !dst_local_dev || !sources_dev || !src_slot_dev) return TKMK_ERR_INVALID_POINTER;
    if (n > (0x7FFFFFFFull << 8)) return TKMK_ERR_INVALID_ARGUMENT;   // one workgroup per 256 entries
    return witness_check_copy_run(CopyCellsSplit{(const fr_t *)b_local_dev, (const fr_t *)sources_dev, local_cells, n_sources, dst_local_dev, src_slot_dev}, n,
                                  bad_entries_out, first_bad_entry_out, stream);
}
