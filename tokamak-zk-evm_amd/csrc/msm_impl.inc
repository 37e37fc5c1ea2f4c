// msm_impl.inc — G1 multi-scalar multiplication (Pippenger bucket method) for gfx950 behind
// bls12_381_msm (include/tkmk.h).  Work-alike of icicle_core::msm::msm as the reference calls it
// (packages/backend/libs/src/iotools/mod.rs:2093-2099 encode_poly; group_structures/mod.rs:108-143).
//
// Pipeline (all on one stream, no host round trip until the W window sums come back):
//   k_convert_bases   plain affine -> Montgomery affine, once per call (skipped for Montgomery input)
//   k_digits          scalar -> W signed c-bit digits (|d| <= 2^(c-1)), coalesced [w][i] u32 records
//   k_hist            per (window, chunk) workgroup: LDS-privatised bucket histogram (<= 128 KiB of LDS)
//   k_scan_local/apply  chunk-exclusive cursors + bucket start offsets (two-level scan over 1024-bucket groups)
//   k_scatter         per (window, chunk): LDS cursors, ds_add_rtn ranks -> bucket-sorted point indices
//   k_accumulate_chunks  one lane per 64-entry chunk of the sorted list: XYZZ accumulator in VGPRs += gathered
//                     affine bases (8M+2S each); k_combine / k_combine_big sum each bucket's chunk fragments
//   k_reduce_segments / k_reduce_windows   sum_v v*B_v per window via 8-bucket running sums
//   host              Horner over the W window sums (W*c doublings) + one inversion -> canonical result
// Sorting by bucket instead of atomically adding points: there are no 384-bit atomics, and the sorted
// order makes each bucket a private serial chain with no inter-lane communication.
//
// Bound: integer VALU (v_mad_u64_u32): ~4.8e4 mul-adds per point-window vs 128 B of traffic; not HBM,
// and MFMA is not applicable (SURVEY.md §8d).
// This file is curve-generic and is included once per curve (msm.hip: BLS12-381, the reference's curve;
// msm_bn254.hip: BN254, named only by BASELINE.json's configs) with
//   TK_MSM_NS            namespace of the instantiation
//   TK_MSM_FR_PARAMS / TK_MSM_FQ_PARAMS   field constants (field_params.h)
//   TK_MSM_SCALAR_BITS   default scalar width (255 / 254)
//   TK_MSM_ABI_FR / _AFFINE / _PROJ / _JOB   C-ABI types, TK_MSM_SYM_MSM / TK_MSM_SYM_MULTI   exported names
namespace TK_MSM_NS {

using FrP = TK_MSM_FR_PARAMS;
using FqP = TK_MSM_FQ_PARAMS;
using Fr = ff<FrP>;
using Fq = ff<FqP>;
using fr_t = Fr::E;
using fq_t = Fq::E;
using G1 = ec<Fq>;
using g1_affine_t = affine_t<Fq>;
using g1_xyzz_t = xyzz_t<Fq>;
using G1U = ecu<FqP>;
// curve arithmetic of the small latency-bound kernels (combine / reduce / size-1): saturated ec.h, fully inlined
using G1K = G1;
using FqK = Fq;
using g1k_xyzz = g1_xyzz_t;
using g1k_aff = g1_affine_t;
using abi_fr = TK_MSM_ABI_FR;
using abi_affine = TK_MSM_ABI_AFFINE;
using abi_proj = TK_MSM_ABI_PROJ;
using abi_job = TK_MSM_ABI_JOB;
#ifdef TK_MSM_SYM_MULTI_EX
using abi_job_ex = TK_MSM_ABI_JOB_EX;
#endif
constexpr size_t AFF_BYTES = sizeof(g1_affine_t), FR_BYTES = sizeof(fr_t);
#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
// row of a TKMK_BASES_ACC_READY table (ec_u.h)
using acc_row_t = G1U::Row;
constexpr size_t ACC_ROW_BYTES = sizeof(acc_row_t);
static_assert(ACC_ROW_BYTES == 128 && alignof(acc_row_t) == 128, "one row per 128-byte line");
#else
struct acc_row_t;   // no accumulate-ready tables for this curve
#endif

static_assert(sizeof(g1_affine_t) == 2 * 4 * Fq::N && sizeof(g1_xyzz_t) == 4 * 4 * Fq::N, "layout");
static_assert(sizeof(abi_fr) == FR_BYTES && sizeof(abi_affine) == AFF_BYTES && sizeof(abi_proj) == 3 * 4 * Fq::N, "ABI layout");
static_assert(Fr::N == 8, "k_digits reads 8 scalar limbs");

struct msm_plan_t {
    uint32_t n;        // points
    uint32_t c;        // window bits
    uint32_t W;        // windows
    uint32_t B;        // buckets per window = 2^(c-1)
    uint32_t chunks;   // histogram chunks per window
    uint32_t chunk_len;
    uint32_t bits;
    // precomputed bases (precompute_factor F > 1): n = n_src * F expanded points [j][i] = 2^(c W j) P_i, W windows per
    // group; the scalar's window w = j W + t lands in window t on point (j, i).  F = 1: n_src = n, W_src = W.
    uint32_t n_src;    // scalars
    uint32_t W_src;    // windows of one scalar = bits / c + 1
    uint32_t chunk;    // entries of the sorted list one accumulate lane sums (chosen per call: see msm_choose_chunk)
    uint32_t win_parts;  // partial sums per window left to the host (k_reduce_windows)
    // single-bucket-set jobs (W = 1, commit table): the weighted bucket sum through row / column sums (k_reduce_rows ...);
    // 0 = the segment reduction.  Buckets are seen as a hi x lo matrix, lo = 2^lo_bits columns
    uint32_t hi_bits, lo_bits;
    uint32_t big;      // a bucket with more fragments than this is summed by a workgroup (k_combine_big) instead of one lane
};

// Operand views (tkmk_msm_multi_ex): point k of an MSM reads scalar sview(k) and base bview(k) of resident tables, so that the
// commit of a coefficient box against a CRS sub-grid (encode_poly, libs/src/iotools/mod.rs:2061-2088) or of gathered wires
// against a binding table (msm_g1_bases, libs/src/group_structures/mod.rs:127-143) needs no gathered copy of either operand.
//   cols != 0 : k -> (k / cols) * stride + k % cols   (a cols-wide box of a stride-wide row-major matrix)
//   index     : k -> index[k]                          (takes precedence; bases only)
// limit = records addressable behind the table: an index at or past it is clamped to 0 and reported through *flag.
struct msm_view_t {
    const uint32_t *index;
    uint32_t cols, stride;
    uint32_t limit;
    uint32_t *flag;
};
__device__ __forceinline__ uint32_t view_at(const msm_view_t &v, uint32_t k) {
    uint32_t r = k;
    if (v.index) r = v.index[k];
    else if (v.cols) {
        uint32_t row = k / v.cols;
        r = row * v.stride + (k - row * v.cols);
    }
    if (v.limit && r >= v.limit) {
        if (v.flag) atomicOr(v.flag, 1u);
        r = 0;
    }
    return r;
}
// precomputed tables (factor F > 1): expanded point k = j * n_src + i is row j * level_rows + view(i) of a table that holds
// level_rows rows per level j (level j = the 2^(c W j) multiples of level 0); level_rows = 0: the expanded points are their own
// table (bls12_381_msm_precompute_bases of exactly this MSM's bases), row k
__device__ __forceinline__ uint32_t view_at_expanded(const msm_view_t &v, uint32_t k, uint32_t n_src, uint32_t level_rows) {
    if (!level_rows) return view_at(v, k);
    uint32_t j = k / n_src;
    return j * level_rows + view_at(v, k - j * n_src);
}
static inline msm_view_t view_identity() { return msm_view_t{nullptr, 0, 0, 0, nullptr}; }
static inline bool view_is_identity(const msm_view_t &v) { return !v.index && !v.cols; }

// bases -> the form the accumulate loop consumes: {x R' mod p, y R' mod p} with R' = 2^(WU LU) (canonical, 32-bit limbs; the
// Montgomery radix of the unsaturated representation, ffu.h); (0,0) stays (0,0) = infinity
__global__ __launch_bounds__(256) void k_convert_bases(const g1_affine_t *__restrict__ in, g1_affine_t *__restrict__ out,
                                                      uint64_t n, int in_montgomery, msm_view_t bv) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1_affine_t p = tk_load(in + view_at(bv, (uint32_t)i));
    if (!G1::is_inf(p)) {
        fq_t k;
#pragma unroll
        for (int j = 0; j < Fq::N; j++) k.l[j] = in_montgomery ? FqP::KSATM[j] : FqP::KSAT[j];
        p.x = Fq::mul(Fq::canon(p.x), k);
        p.y = Fq::mul(Fq::canon(p.y), k);
    }
    tk_store(out + i, p);
}

// digit record: bit 31 = negative, low bits = |d| in [1, B]; 0 = skip
__global__ __launch_bounds__(256) void k_digits(const fr_t *__restrict__ scalars, uint32_t *__restrict__ dig, msm_plan_t pl,
                                               int scalars_mont, msm_view_t sv) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pl.n_src) return;
    fr_t s = Fr::canon(tk_load(scalars + view_at(sv, i)));
    if (scalars_mont) s = Fr::from_mont(s);
    uint32_t carry = 0;
    const uint32_t mask = (1u << pl.c) - 1u;
    const uint32_t groups = pl.n / pl.n_src;   // precompute factor
    uint32_t j = 0, t = 0;                     // window w = j * pl.W + t
    for (uint32_t w = 0; w < groups * pl.W; w++) {
        if (w >= pl.W_src) {                   // padding windows of the last group
            dig[(uint64_t)t * pl.n + (uint64_t)j * pl.n_src + i] = 0;
            if (++t == pl.W) { t = 0; j++; }
            continue;
        }
        uint32_t lo = w * pl.c, li = lo >> 5, sh = lo & 31;
        uint32_t raw = 0;
        if (li < 8) {
            raw = s.l[li] >> sh;
            if (sh + pl.c > 32 && li + 1 < 8) raw |= s.l[li + 1] << (32 - sh);
        }
        raw &= mask;
        if (lo + pl.c > pl.bits) {  // drop bits above `bits`
            uint32_t keep = pl.bits > lo ? pl.bits - lo : 0;
            raw &= keep >= 32 ? 0xffffffffu : ((1u << keep) - 1u);
        }
        uint32_t v = raw + carry;
        uint32_t rec;
        if (v > pl.B) {
            rec = ((1u << pl.c) - v) | 0x80000000u;
            carry = 1;
        } else {
            rec = v;
            carry = 0;
        }
        dig[(uint64_t)t * pl.n + (uint64_t)j * pl.n_src + i] = rec;
        if (++t == pl.W) { t = 0; j++; }
    }
}

// expanded base table of the precompute mode: out[j * n + i] = 2^(step * j) P_i in the converted form of k_convert_bases
// (x R', y R' packed), j < factor; one lane per point, one inversion per table entry (a one-time cost per CRS)
template <class Out>
__device__ __forceinline__ void precompute_bases_body(const g1_affine_t *__restrict__ in, Out *__restrict__ out, uint64_t n, int in_montgomery,
                                                      uint32_t factor, uint32_t step) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1_affine_t p = tk_load(in + i);
    const bool inf = G1::is_inf(p);
    if (!inf) {
        p.x = Fq::canon(p.x);
        p.y = Fq::canon(p.y);
        if (!in_montgomery) {
            p.x = Fq::to_mont(p.x);
            p.y = Fq::to_mont(p.y);
        }
    }
    fq_t k;
#pragma unroll
    for (int l = 0; l < Fq::N; l++) k.l[l] = FqP::KSATM[l];
    g1_xyzz_t acc = G1::from_affine(p);
    for (uint32_t j = 0; j < factor; j++) {
        g1_affine_t a = p;
        if (j) {
            for (uint32_t d = 0; d < step; d++) acc = G1::dbl(acc);
            a = G1::to_affine(acc);
        }
        if (!inf) {
            a.x = Fq::mul(a.x, k);
            a.y = Fq::mul(a.y, k);
        }
        Out rec;
        G1U::to_record(rec, a);
        tk_store(out + (uint64_t)j * n + i, rec);
    }
}
__global__ __launch_bounds__(128) void k_precompute_bases(const g1_affine_t *__restrict__ in, g1_affine_t *__restrict__ out, uint64_t n,
                                                         int in_montgomery, uint32_t factor, uint32_t step) {
    precompute_bases_body(in, out, n, in_montgomery, factor, step);
}
#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
// the same table as accumulate-ready rows (ec_u.h), written directly: no second pass over the table
__global__ __launch_bounds__(128) void k_precompute_bases_acc(const g1_affine_t *__restrict__ in, acc_row_t *__restrict__ out, uint64_t n,
                                                             int in_montgomery, uint32_t factor, uint32_t step) {
    precompute_bases_body(in, out, n, in_montgomery, factor, step);
}
#endif

// grid (chunks, W); dynamic LDS = B * 4 bytes
__global__ __launch_bounds__(1024) void k_hist(const uint32_t *__restrict__ dig, uint32_t *__restrict__ counts, msm_plan_t pl,
                                              uint32_t shift) {
    extern __shared__ uint32_t hist[];
    const uint32_t w = blockIdx.y, ch = blockIdx.x;
    for (uint32_t b = threadIdx.x; b < pl.B; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    uint32_t lo = ch * pl.chunk_len, hi = lo + pl.chunk_len;
    if (hi > pl.n) hi = pl.n;
    const uint32_t *d = dig + (uint64_t)w * pl.n;
    uint32_t i = lo + threadIdx.x;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {   // four independent loads in flight: the loop is load-latency bound
        uint32_t r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = d[i + 1024 * j] & 0x7fffffffu;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (r[j]) atomicAdd(&hist[(r[j] - 1) >> shift], 1u);
    }
    for (; i < hi; i += 1024) {
        uint32_t r = d[i] & 0x7fffffffu;
        if (r) atomicAdd(&hist[(r - 1) >> shift], 1u);
    }
    __syncthreads();
    // counts[w][b][chunk]
    uint32_t *c = counts + (uint64_t)w * pl.B * pl.chunks;
    for (uint32_t b = threadIdx.x; b < pl.B; b += blockDim.x) c[(uint64_t)b * pl.chunks + ch] = hist[b];
}

// counts[w][b][chunk] -> exclusive cursors (absolute position in the window's sorted list) and bstart[w][b],
// b in [0, B], in two launches over (ceil(B/1024), W) workgroups:
//   k_scan_local : one lane per bucket sums its chunks; workgroup-exclusive scan; group total -> gtot[w][grp]
//   k_scan_apply : adds the exclusive prefix of the (<= 32) group totals, writes bstart and the cursors
__global__ __launch_bounds__(1024) void k_scan_local(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local,
                                                    uint32_t *__restrict__ gtot, msm_plan_t pl) {
    __shared__ uint32_t part[1024];
    const uint32_t w = blockIdx.y, t = threadIdx.x, b = blockIdx.x * 1024 + t;
    uint32_t sum = 0;
    if (b < pl.B) {
        const uint32_t *c = counts + ((uint64_t)w * pl.B + b) * pl.chunks;
        uint32_t k = 0;
        for (; k + 8 <= pl.chunks; k += 8) {   // eight loads in flight: with 512 chunks and one block per window this loop is pure load latency
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = c[k + j];
#pragma unroll
            for (int j = 0; j < 8; j++) sum += v[j];
        }
        for (; k < pl.chunks; k++) sum += c[k];
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        uint32_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (b < pl.B) local[(uint64_t)w * pl.B + b] = part[t] - sum;  // exclusive within the group
    if (t == 1023) gtot[w * gridDim.x + blockIdx.x] = part[t];
}
__global__ __launch_bounds__(1024) void k_scan_apply(uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                    const uint32_t *__restrict__ gtot, uint32_t *__restrict__ bstart, msm_plan_t pl) {
    const uint32_t w = blockIdx.y, t = threadIdx.x, b = blockIdx.x * 1024 + t;
    uint32_t base = 0, total = 0;
    for (uint32_t g = 0; g < gridDim.x; g++) {
        uint32_t v = gtot[w * gridDim.x + g];
        if (g < blockIdx.x) base += v;
        total += v;
    }
    uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
    if (b < pl.B) {
        uint32_t run = base + local[(uint64_t)w * pl.B + b];
        bs[b] = run;
        uint32_t *c = counts + ((uint64_t)w * pl.B + b) * pl.chunks;
        uint32_t k = 0;
        for (; k + 8 <= pl.chunks; k += 8) {
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = c[k + j];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                c[k + j] = run;
                run += v[j];
            }
        }
        for (; k < pl.chunks; k++) {
            uint32_t v = c[k];
            c[k] = run;
            run += v;
        }
    }
    if (blockIdx.x == 0 && t == 0) bs[pl.B] = total;
}

// The same two steps for few windows and many chunks (the commit table: ONE window, 1024 coarse bins x 512 chunks): with one thread
// per bin a single workgroup walks 512 counts per thread, 64 dependent load batches in each kernel (0.2 ms per commit).  Here 16
// lanes share a bin (a contiguous 1/16 of its chunks each) and 64 bins share a workgroup: grid (B / 64, W).
#define SCW_TPB 16
#define SCW_BINS (1024 / SCW_TPB)
__global__ __launch_bounds__(1024) void k_scan_local_wide(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local,
                                                         uint32_t *__restrict__ gtot, msm_plan_t pl) {
    __shared__ uint32_t binsum[SCW_BINS];
    const uint32_t w = blockIdx.y, t = threadIdx.x, slot = t / SCW_TPB, sub = t % SCW_TPB, b = blockIdx.x * SCW_BINS + slot;
    const uint32_t per = (pl.chunks + SCW_TPB - 1) / SCW_TPB, lo = sub * per, hi = lo + per < pl.chunks ? lo + per : pl.chunks;
    uint32_t sum = 0;
    if (b < pl.B) {
        const uint32_t *c = counts + ((uint64_t)w * pl.B + b) * pl.chunks;
        for (uint32_t k = lo; k < hi; k++) sum += c[k];
    }
#pragma unroll
    for (uint32_t off = SCW_TPB / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, SCW_TPB);
    if (sub == 0) binsum[slot] = sum;
    __syncthreads();
    if (t < SCW_BINS) {   // one wave: inclusive scan of the 64 bin sums
        uint32_t mine = binsum[t], incl = mine;
#pragma unroll
        for (uint32_t off = 1; off < SCW_BINS; off <<= 1) {
            uint32_t v = __shfl_up(incl, off, SCW_BINS);
            if (t >= off) incl += v;
        }
        const uint32_t bb = blockIdx.x * SCW_BINS + t;
        if (bb < pl.B) local[(uint64_t)w * pl.B + bb] = incl - mine;
        if (t == SCW_BINS - 1) gtot[w * gridDim.x + blockIdx.x] = incl;
    }
}
__global__ __launch_bounds__(1024) void k_scan_apply_wide(uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                         const uint32_t *__restrict__ gtot, uint32_t *__restrict__ bstart, msm_plan_t pl) {
    const uint32_t w = blockIdx.y, t = threadIdx.x, slot = t / SCW_TPB, sub = t % SCW_TPB, b = blockIdx.x * SCW_BINS + slot;
    const uint32_t per = (pl.chunks + SCW_TPB - 1) / SCW_TPB, lo = sub * per, hi = lo + per < pl.chunks ? lo + per : pl.chunks;
    uint32_t base = 0, total = 0;
    for (uint32_t g = 0; g < gridDim.x; g++) {
        uint32_t v = gtot[w * gridDim.x + g];
        if (g < blockIdx.x) base += v;
        total += v;
    }
    uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
    uint32_t *c = counts + ((uint64_t)w * pl.B + (b < pl.B ? b : 0)) * pl.chunks;
    uint32_t sum = 0;
    if (b < pl.B)
        for (uint32_t k = lo; k < hi; k++) sum += c[k];
    uint32_t incl = sum;   // prefix of the 16 lanes' ranges inside the bin
#pragma unroll
    for (uint32_t off = 1; off < SCW_TPB; off <<= 1) {
        uint32_t v = __shfl_up(incl, off, SCW_TPB);
        if (sub >= off) incl += v;
    }
    if (b < pl.B) {
        const uint32_t bin_start = base + local[(uint64_t)w * pl.B + b];
        if (sub == 0) bs[b] = bin_start;
        uint32_t run = bin_start + incl - sum;
        for (uint32_t k = lo; k < hi; k++) {
            uint32_t v = c[k];
            c[k] = run;
            run += v;
        }
    }
    if (blockIdx.x == 0 && t == 0) bs[pl.B] = total;
}

// grid (chunks, W); dynamic LDS = B * 4 bytes.  sorted[w][pos] = point index | sign
__global__ __launch_bounds__(1024) void k_scatter(const uint32_t *__restrict__ dig, const uint32_t *__restrict__ counts,
                                                 uint32_t *__restrict__ sorted, msm_plan_t pl, msm_view_t bv, uint32_t level_rows) {
    extern __shared__ uint32_t cur[];
    const uint32_t w = blockIdx.y, ch = blockIdx.x;
    const uint32_t *c = counts + (uint64_t)w * pl.B * pl.chunks;
    for (uint32_t b = threadIdx.x; b < pl.B; b += blockDim.x) cur[b] = c[(uint64_t)b * pl.chunks + ch];
    __syncthreads();
    uint32_t lo = ch * pl.chunk_len, hi = lo + pl.chunk_len;
    if (hi > pl.n) hi = pl.n;
    const uint32_t *d = dig + (uint64_t)w * pl.n;
    uint32_t *s = sorted + (uint64_t)w * pl.n;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint32_t rec = d[i];
        uint32_t r = rec & 0x7fffffffu;
        if (r) {
            uint32_t pos = atomicAdd(&cur[r - 1], 1u);
            s[pos] = view_at_expanded(bv, i, pl.n_src, level_rows) | (rec & 0x80000000u);   // the sorted lists hold base-table rows
        }
    }
}

// ---- two-pass (MSD) bucket sort with LDS-staged, coalesced scatters -----------------------------------------
// The single-pass k_scatter issues one 4-byte store per item into 2^15 x chunks different 64-byte granules: 2^28
// partial-line writes that the L2 / fabric retire at ~40 G/s chip-wide (6.6 ms at 2^24 points, 8x write
// amplification).  Splitting the bucket index into a coarse part (<= 256 bins) and a fine part (128 bins) lets
// each pass sort a 4096-item tile by bin inside LDS first, so that a wave writes runs of consecutive addresses.
//   pass A: per (chunk, window): bins = bucket >> f;  out: A_idx = point | sign, A_key = bucket & (2^f - 1), grouped by coarse bin
//   pass B: per (part, (window, coarse bin)): bins = A_key;  out: the final bucket-sorted index list       (f = 7 or 8)
// (r4: 8192-item tiles — twice as long runs per bin, 76 KB of LDS, still two workgroups per CU — measured: the two passes take 14.3 ms per
// configs[3] proof either way; the passes are bound by their barriers and LDS round trips, not by the length of the runs they write)
#ifndef SC_TILE
#define SC_TILE 4096
#endif
#define SC_PER (SC_TILE / 1024)   // items per thread and tile
#define SC_MAXBINS 1024  // bins per pass: coarse <= 1024, fine <= 512 (c <= 20: 2^19 buckets = 1024 x 512)
#define SC_MAXFINE 512
#define SC_PARTS 4
// a segment (pass B: one (window, coarse bin) range) is cut into `parts` ranges of whole tiles: a 4096-item segment (2^20
// points) is ONE full tile for part 0 and nothing for the others, instead of four quarter-filled tiles that each pay the
// tile's fixed cost (histogram, 512-lane scan, barriers); a giant segment (witness-like scalars) still splits evenly
__device__ __forceinline__ uint32_t sc_part_len(uint32_t len, uint32_t parts) {
    uint32_t per = (len + parts - 1) / parts;
    return (per + SC_TILE - 1) / SC_TILE * SC_TILE;
}

template <bool PASS_B>
__global__ __launch_bounds__(1024) void k_scatter_staged(const uint32_t *__restrict__ in0, const uint16_t *__restrict__ in1,
                                                        const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ cursors,
                                                        uint32_t *__restrict__ out0, uint16_t *__restrict__ out1, uint32_t n,
                                                        uint32_t bins, uint32_t coarse_bins, uint32_t chunk_len, uint32_t fbits,
                                                        msm_view_t bv, uint32_t n_src, uint32_t level_rows) {
    __shared__ uint32_t hist[SC_MAXBINS], start[SC_MAXBINS], cur[SC_MAXBINS], wsum[16];
    const uint32_t fmask = (1u << fbits) - 1;
    __shared__ uint32_t sv0[SC_TILE], sv1[SC_TILE];
    const uint32_t tid = threadIdx.x, parts = gridDim.x, sgm = blockIdx.y;
    // XCD-aware part assignment: workgroups go to the 8 XCDs round-robin by linear id, and the runs that consecutive parts write
    // into one bin are adjacent in memory (16-32 bytes each).  Give every XCD a contiguous range of parts, so the pieces of a
    // 128-byte line meet in ONE L2 before they are written back instead of arriving as partial lines from eight
    uint32_t part = blockIdx.x;
    if ((parts & 7u) == 0) part = (blockIdx.x & 7u) * (parts >> 3) + (blockIdx.x >> 3);
    const uint32_t w = PASS_B ? sgm / coarse_bins : sgm;
    uint32_t lo, hi, base = 0;
    if (PASS_B) {
        const uint32_t cb = sgm - w * coarse_bins;
        const uint32_t *cs = seg_start + (uint64_t)w * (coarse_bins + 1);
        uint32_t s0 = cs[cb], s1 = cs[cb + 1];
        uint32_t per = sc_part_len(s1 - s0, parts);
        lo = s0 + part * per;
        if (lo > s1) lo = s1;
        hi = lo + per < s1 ? lo + per : s1;
        base = s0;
    } else {
        lo = part * chunk_len;
        hi = lo + chunk_len < n ? lo + chunk_len : n;
        if (lo > n) lo = n;
    }
    in0 += (uint64_t)w * n;
    if (PASS_B) in1 += (uint64_t)w * n;
    out0 += (uint64_t)w * n;
    if (!PASS_B) out1 += (uint64_t)w * n;
    if (tid < bins) cur[tid] = cursors[((uint64_t)sgm * bins + tid) * parts + part] + base;
    hist[tid] = 0;
    __syncthreads();
    for (uint32_t tlo = lo; tlo < hi; tlo += SC_TILE) {
        uint32_t v0[SC_PER], v1[SC_PER], rk[SC_PER];
        bool ok[SC_PER];
#pragma unroll
        for (int j = 0; j < SC_PER; j++) {
            uint32_t k = tlo + tid + 1024u * j;
            ok[j] = k < hi;
            v0[j] = v1[j] = rk[j] = 0;
            if (ok[j]) {
                if (PASS_B) {
                    v0[j] = in0[k];
                    v1[j] = in1[k];
                } else {
                    uint32_t rec = in0[k], r = rec & 0x7fffffffu;
                    ok[j] = r != 0;
                    v0[j] = (ok[j] ? view_at_expanded(bv, k, n_src, level_rows) : 0u) | (rec & 0x80000000u);   // base-table row of point k
                    v1[j] = r - 1;
                }
            }
            if (ok[j]) rk[j] = atomicAdd(&hist[PASS_B ? (v1[j] & fmask) : (v1[j] >> fbits)], 1u);
        }
        __syncthreads();
        // exclusive prefix of hist[] -> start[]: scan inside each wave with lane shuffles, then the 16 wave totals (two barriers
        // per tile; the former Hillis-Steele over LDS took twenty)
        static_assert(SC_MAXBINS == 1024, "one bin per thread of the 1024-thread workgroup");
        const uint32_t mine = hist[tid];
        uint32_t incl = mine;
        const uint32_t lane = tid & 63u, wave = tid >> 6;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w2 = 0; w2 < 16; w2++) {
            uint32_t v = wsum[w2];
            total += v;
            if (w2 < wave) before += v;
        }
        start[tid] = before + incl - mine;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SC_PER; j++)
            if (ok[j]) {
                uint32_t b = PASS_B ? (v1[j] & fmask) : (v1[j] >> fbits);
                uint32_t pos = start[b] + rk[j];
                sv0[pos] = v0[j];
                sv1[pos] = v1[j];
            }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SC_PER; j++) {
            uint32_t k2 = tid + 1024u * j;
            if (k2 < total) {
                uint32_t a0 = sv0[k2], a1 = sv1[k2];
                uint32_t b = PASS_B ? (a1 & fmask) : (a1 >> fbits);
                uint32_t g = cur[b] + (k2 - start[b]);
                out0[g] = a0;
                if (!PASS_B) out1[g] = (uint16_t)(a1 & fmask);   // pass B only needs the fine part
            }
        }
        __syncthreads();
        cur[tid] += hist[tid];   // and clear the histogram for the next tile: same element, same thread
        hist[tid] = 0;
        __syncthreads();
    }
}

// pass-B histogram: counts[(w * coarse_bins + cb)][fine][part]
__global__ __launch_bounds__(1024) void k_hist_fine(const uint16_t *__restrict__ key, const uint32_t *__restrict__ seg_start,
                                                   uint32_t *__restrict__ counts, uint32_t n, uint32_t coarse_bins, uint32_t fbits) {
    __shared__ uint32_t hist[SC_MAXFINE];
    const uint32_t fb_n = 1u << fbits;
    const uint32_t tid = threadIdx.x, part = blockIdx.x, parts = gridDim.x, sgm = blockIdx.y;
    const uint32_t w = sgm / coarse_bins, cb = sgm - w * coarse_bins;
    const uint32_t *cs = seg_start + (uint64_t)w * (coarse_bins + 1);
    uint32_t s0 = cs[cb], s1 = cs[cb + 1];
    uint32_t per = sc_part_len(s1 - s0, parts);
    uint32_t lo = s0 + part * per;
    if (lo > s1) lo = s1;
    uint32_t hi = lo + per < s1 ? lo + per : s1;
    if (tid < fb_n) hist[tid] = 0;
    __syncthreads();
    const uint16_t *k = key + (uint64_t)w * n;
    uint32_t i = lo + tid;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {
        uint32_t r[4];
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = k[i + 1024 * j];
#pragma unroll
        for (int j = 0; j < 4; j++) atomicAdd(&hist[r[j] & (fb_n - 1)], 1u);
    }
    for (; i < hi; i += 1024) atomicAdd(&hist[k[i] & (fb_n - 1)], 1u);
    __syncthreads();
    if (tid < fb_n) counts[((uint64_t)sgm * fb_n + tid) * parts + part] = hist[tid];
}

// bstart[w][cb * 128 + fb] = coarse_start[w][cb] + fine_start[w * CB + cb][fb];  bstart[w][B] = total
__global__ __launch_bounds__(256) void k_bstart_assemble(const uint32_t *__restrict__ coarse_start, const uint32_t *__restrict__ fine_start,
                                                        uint32_t *__restrict__ bstart, uint32_t W, uint32_t B, uint32_t coarse_bins,
                                                        uint32_t fbits) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)W * (B + 1)) return;
    uint32_t w = (uint32_t)(e / (B + 1)), b = (uint32_t)(e - (uint64_t)w * (B + 1));
    const uint32_t *cs = coarse_start + (uint64_t)w * (coarse_bins + 1);
    if (b == B) {
        bstart[e] = cs[coarse_bins];
        return;
    }
    uint32_t cb = b >> fbits, fb = b & ((1u << fbits) - 1);
    bstart[e] = cs[cb] + fine_start[((uint64_t)w * coarse_bins + cb) * ((1u << fbits) + 1) + fb];
}

// adds the windows' sorted-list lengths (bstart[w][B]) to the library's "bucket additions issued" cell
__global__ void k_count_entries(const uint32_t *__restrict__ bstart, uint32_t W, uint32_t B, unsigned long long *__restrict__ cell) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < W; w++) t += bstart[(uint64_t)w * (B + 1) + B];
    atomicAdd(cell, t);
}

// ---- bucket accumulation, balanced by construction -------------------------------------------------
// The window's bucket-sorted list is cut into chunks of MSM_CHUNK consecutive entries and every lane sums
// exactly one chunk (an XYZZ accumulator in VGPRs += gathered affine base, 8M + 2S per entry), whatever
// the bucket sizes are: real prover inputs are heavily skewed (witness wires are mostly 0/1: SURVEY.md
// Appendix B) and one-lane-per-bucket would serialise a 10^5-entry bucket on a single lane.
// A chunk intersects buckets in at most: one HEAD fragment (a bucket that covers the chunk start but is not
// wholly inside the chunk), any number of whole buckets (written straight to buckets[]), one TAIL fragment
// (a bucket that starts inside and runs past the chunk end).  k_combine then sums each bucket's fragments
// (tail of its first chunk, heads of the following chunks); buckets with more than MSM_BIG fragments are
// queued for k_combine_big (one workgroup per bucket, LDS tree).
#define MSM_CHUNK 64   // target length; the length used by a call is msm_plan_t::chunk
#define MSM_BIG 12   // (r4: 48 before — a lane summing 48 fragments is a 0.6 ms chain, the whole of k_combine for the prover's sparse commits; serialised combine 8.7 -> 8.0 ms per proof)
// buckets with more than MSM_GIANT fragments (> 131072 entries: the "wire = 1" bucket of a witness MSM holds millions)
// are summed by MSM_GIANT_PARTS workgroups each and a second small kernel instead of one workgroup
#define MSM_GIANT 2048
#define MSM_GIANT_PARTS 32
#define MSM_GIANT_CAP 2048

__device__ __forceinline__ uint32_t bucket_of(const uint32_t *__restrict__ bs, uint32_t B, uint32_t pos) {
    // largest b in [0, B) with bs[b] <= pos  (bs is non-decreasing, bs[0] = 0)
    uint32_t lo = 0, hi = B;
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (bs[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Row = g1_affine_t: the packed 96-byte converted record (every MSM but the table jobs of TKMK_BASES_ACC_READY); Row = acc_row_t: the
// 128-byte accumulate-ready row of a resident commit table — the row number in the sorted record is the same, the stride and the loader
// differ, and the sign of the entry goes into the addition instead of a negated copy of the base.
template <class Row>
__device__ __forceinline__ void accumulate_chunks_body(const Row *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                       const uint32_t *__restrict__ bstart, g1_xyzz_t *__restrict__ buckets,
                                                       g1_xyzz_t *__restrict__ frag_head, g1_xyzz_t *__restrict__ frag_tail,
                                                       const msm_plan_t &pl, uint32_t chunks_per_window) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= pl.W * chunks_per_window) return;
    uint32_t w = gid / chunks_per_window, t = gid - w * chunks_per_window;
    const uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
    const uint32_t total = bs[pl.B];
    uint32_t lo = t * pl.chunk;
    if (lo >= total) return;
    uint32_t hi = lo + pl.chunk < total ? lo + pl.chunk : total;
    const uint32_t *s = sorted + (uint64_t)w * pl.n;
    uint32_t b = bucket_of(bs, pl.B, lo);
    uint32_t bend = bs[b + 1];           // end of the current bucket (> lo by construction of bucket_of,
    while (bend <= lo) bend = bs[++b + 1];  //  except across empty buckets sharing the same offset)
    // bucket boundaries are fetched one bucket ahead and the current bucket's start is tracked in registers: inside the
    // (divergent) flush branch nothing waits on a load — with 32-entry buckets some lane of the wave flushes almost every iteration
    const bool first_starts_here = bs[b] == lo;
    uint32_t nb = b + 2 <= pl.B ? bs[b + 2] : 0xffffffffu;   // end of the next bucket
    uint32_t seg_lo = lo;
    G1U::X acc = G1U::inf();
    // Software pipeline of the gather: the base row of entry k + 1 is requested before the addition of entry k starts (its sorted-list
    // record was requested an iteration earlier still), so the ~2 dependent memory latencies of an entry run under ~10 us of
    // multiply-adds instead of in front of them.  (With every gather hitting the cache the kernel is 12.7 % faster: that is what the
    // two waves per SIMD do not hide by themselves.)
    uint32_t rec_next = s[lo], rec_next2 = lo + 1 < hi ? s[lo + 1] : 0u;
    Row raw = tk_load(bases + (rec_next & 0x7fffffffu));
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t rec = rec_next;
        G1U::A q;
        bool have;
        if constexpr (std::is_same<Row, g1_affine_t>::value) have = G1U::load_affine(q, raw);
        else have = G1U::load_row(q, raw);
        rec_next = rec_next2;
        if (k + 1 < hi) {
            raw = tk_load(bases + (rec_next & 0x7fffffffu));
        }
        if (k + 2 < hi) rec_next2 = s[k + 2];
        if (have) {
            if constexpr (std::is_same<Row, g1_affine_t>::value) {
                if (rec & 0x80000000u) q = G1U::neg(q);
                acc = G1U::add_mixed(acc, q);
            } else {
                acc = G1U::add_mixed_masked(acc, q, (uint32_t)((int32_t)rec >> 31));   // sign bit of the record -> mask
            }
        }
        if (k + 1 == bend || k + 1 == hi) {  // the segment [seg_lo, k+1) of bucket b ends here
            bool whole = (seg_lo != lo || first_starts_here) && k + 1 == bend;   // a bucket begun in this chunk begins at seg_lo
            g1_xyzz_t *dst;
            if (whole) dst = buckets + (uint64_t)w * pl.B + b;
            else if (seg_lo == lo) dst = frag_head + (uint64_t)w * chunks_per_window + t;
            else dst = frag_tail + (uint64_t)w * chunks_per_window + t;
            tk_store(dst, G1U::to_raw(acc));   // no products here: this branch is divergent (see ec_u.h)
            acc = G1U::inf();
            seg_lo = k + 1;
            if (k + 1 < hi) {
                do {
                    b++;
                    bend = nb;
                    nb = b + 2 <= pl.B ? bs[b + 2] : 0xffffffffu;
                } while (bend <= k + 1);
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void k_accumulate_chunks(const g1_affine_t *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                          const uint32_t *__restrict__ bstart, g1_xyzz_t *__restrict__ buckets,
                                                          g1_xyzz_t *__restrict__ frag_head, g1_xyzz_t *__restrict__ frag_tail,
                                                          msm_plan_t pl, uint32_t chunks_per_window) {
    accumulate_chunks_body(bases, sorted, bstart, buckets, frag_head, frag_tail, pl, chunks_per_window);
}
#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
__global__ __launch_bounds__(256, 2) void k_accumulate_chunks_rows(const acc_row_t *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                               const uint32_t *__restrict__ bstart, g1_xyzz_t *__restrict__ buckets,
                                                               g1_xyzz_t *__restrict__ frag_head, g1_xyzz_t *__restrict__ frag_tail,
                                                               msm_plan_t pl, uint32_t chunks_per_window) {
    accumulate_chunks_body(bases, sorted, bstart, buckets, frag_head, frag_tail, pl, chunks_per_window);
}
#endif

// one lane per (window, bucket): gather the bucket's fragments.  big[0] = count, big[1 + i] = w * B + b
__global__ __launch_bounds__(256) void k_combine(const uint32_t *__restrict__ bstart, g1_xyzz_t *__restrict__ buckets,
                                                const g1_xyzz_t *__restrict__ frag_head, const g1_xyzz_t *__restrict__ frag_tail,
                                                msm_plan_t pl, uint32_t chunks_per_window, uint32_t *__restrict__ big,
                                                uint32_t big_cap, uint32_t *__restrict__ giant) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= pl.W * pl.B) return;
    uint32_t w = gid / pl.B, b = gid - w * pl.B;
    const uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
    uint32_t sb = bs[b], eb = bs[b + 1];
    if (eb == sb) return;  // buckets[] was zeroed = infinity
    uint32_t t0 = sb / pl.chunk, t1 = (eb - 1) / pl.chunk;
    if (t0 == t1) return;  // wholly inside one chunk: k_accumulate_chunks already wrote the bucket's raw record
    if (t1 - t0 > MSM_GIANT) {
        uint32_t slot = atomicAdd(&giant[0], 1u);
        if (slot < MSM_GIANT_CAP) {
            giant[1 + slot] = gid;
            return;
        }
        // more giants than the cap (cannot happen below 2^28 sorted entries): fall through to the one-workgroup path
    }
    if (t1 - t0 > pl.big) {
        uint32_t slot = atomicAdd(&big[0], 1u);
        if (slot < big_cap) {
            big[1 + slot] = gid;
            return;
        }
        // queue full (it is sized for every bucket, so this is unreachable): sum the fragments here rather than lose the bucket
    }
    const g1_xyzz_t *fh = frag_head + (uint64_t)w * chunks_per_window, *ft = frag_tail + (uint64_t)w * chunks_per_window;
    G1U::X acc = G1U::from_raw(tk_load(sb == t0 * pl.chunk ? fh + t0 : ft + t0));
    for (uint32_t t = t0 + 1; t <= t1; t++) acc = G1U::add(acc, G1U::from_raw(tk_load(fh + t)));
    tk_store(buckets + gid, G1U::to_raw(acc));
}

// grid-stride over the queued big buckets, one WAVE each (four per workgroup): 64 lanes sum strided fragments, 6-level LDS tree.
// (r4: one workgroup per bucket before — 8 tree levels with most lanes idle for the 13..48-fragment buckets this queue mostly holds, and a
// quarter of the buckets in flight; a launch whose buckets are nearly all queued — 16-bit windows — took 5 ms instead of 1.)
__global__ __launch_bounds__(256) void k_combine_big(const uint32_t *__restrict__ bstart, g1_xyzz_t *__restrict__ buckets,
                                                    const g1_xyzz_t *__restrict__ frag_head, const g1_xyzz_t *__restrict__ frag_tail,
                                                    msm_plan_t pl, uint32_t chunks_per_window, const uint32_t *__restrict__ big,
                                                    uint32_t big_cap) {
    __shared__ g1_xyzz_t sh[256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t count = big[0] < big_cap ? big[0] : big_cap;
    for (uint32_t base = blockIdx.x * 4u; base < count; base += gridDim.x * 4u) {   // uniform over the workgroup: the barriers below are reached by all
        const uint32_t i = base + wave;
        const bool live = i < count;
        uint32_t gid = 0;
        G1U::X acc = G1U::inf();
        if (live) {
            gid = big[1 + i];
            uint32_t w = gid / pl.B, b = gid - w * pl.B;
            const uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
            uint32_t sb = bs[b], eb = bs[b + 1];
            uint32_t t0 = sb / pl.chunk, t1 = (eb - 1) / pl.chunk;
            const g1_xyzz_t *fh = frag_head + (uint64_t)w * chunks_per_window, *ft = frag_tail + (uint64_t)w * chunks_per_window;
            for (uint32_t t = t0 + lane; t <= t1; t += 64) {
                const g1_xyzz_t *src = (t == t0 && sb != t0 * pl.chunk) ? ft + t : fh + t;
                acc = G1U::add(acc, G1U::from_raw(tk_load(src)));
            }
        }
        sh[threadIdx.x] = G1U::to_raw(acc);
        __syncthreads();
        for (uint32_t st = 32; st > 0; st >>= 1) {
            if (lane < st) {
                acc = G1U::add(acc, G1U::from_raw(sh[threadIdx.x + st]));
                sh[threadIdx.x] = G1U::to_raw(acc);
            }
            __syncthreads();
        }
        if (live && lane == 0) tk_store(buckets + gid, G1U::to_raw(acc));
        __syncthreads();
    }
}

// giant buckets, stage 1: work item (giant i, part) sums fragments [t0 + part*per, ...) of bucket i into part_out[i][part]
__global__ __launch_bounds__(256) void k_combine_giant_parts(const uint32_t *__restrict__ bstart, const g1_xyzz_t *__restrict__ frag_head,
                                                            const g1_xyzz_t *__restrict__ frag_tail, msm_plan_t pl,
                                                            uint32_t chunks_per_window, const uint32_t *__restrict__ giant,
                                                            g1_xyzz_t *__restrict__ part_out) {
    __shared__ g1_xyzz_t sh[256];
    uint32_t count = giant[0] < MSM_GIANT_CAP ? giant[0] : MSM_GIANT_CAP;
    for (uint32_t item = blockIdx.x; item < count * MSM_GIANT_PARTS; item += gridDim.x) {
        uint32_t i = item / MSM_GIANT_PARTS, part = item - i * MSM_GIANT_PARTS;
        uint32_t gid = giant[1 + i];
        uint32_t w = gid / pl.B, b = gid - w * pl.B;
        const uint32_t *bs = bstart + (uint64_t)w * (pl.B + 1);
        uint32_t sb = bs[b], eb = bs[b + 1];
        uint32_t t0 = sb / pl.chunk, t1 = (eb - 1) / pl.chunk;
        uint32_t per = (t1 - t0 + MSM_GIANT_PARTS) / MSM_GIANT_PARTS;   // ceil((t1 - t0 + 1) / PARTS)
        uint32_t lo = t0 + part * per, hi = lo + per - 1 < t1 ? lo + per - 1 : t1;
        const g1_xyzz_t *fh = frag_head + (uint64_t)w * chunks_per_window, *ft = frag_tail + (uint64_t)w * chunks_per_window;
        G1U::X acc = G1U::inf();
        for (uint32_t t = lo + threadIdx.x; t <= hi && lo <= t1; t += 256) {
            const g1_xyzz_t *src = (t == t0 && sb != t0 * pl.chunk) ? ft + t : fh + t;
            acc = G1U::add(acc, G1U::from_raw(tk_load(src)));
        }
        sh[threadIdx.x] = G1U::to_raw(acc);
        __syncthreads();
        for (uint32_t st = 128; st > 0; st >>= 1) {
            if (threadIdx.x < st) {
                acc = G1U::add(acc, G1U::from_raw(sh[threadIdx.x + st]));
                sh[threadIdx.x] = G1U::to_raw(acc);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) tk_store(part_out + item, G1U::to_raw(acc));
        __syncthreads();
    }
}
// stage 2: bucket = sum of its MSM_GIANT_PARTS partial sums (one wave per giant bucket)
__global__ __launch_bounds__(64) void k_combine_giant_final(g1_xyzz_t *__restrict__ buckets, const uint32_t *__restrict__ giant,
                                                           const g1_xyzz_t *__restrict__ part_in) {
    __shared__ g1_xyzz_t sh[MSM_GIANT_PARTS];
    uint32_t count = giant[0] < MSM_GIANT_CAP ? giant[0] : MSM_GIANT_CAP;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        G1U::X acc = G1U::inf();
        if (threadIdx.x < MSM_GIANT_PARTS) {
            sh[threadIdx.x] = tk_load(part_in + (uint64_t)i * MSM_GIANT_PARTS + threadIdx.x);
            acc = G1U::from_raw(sh[threadIdx.x]);
        }
        __syncthreads();
        for (uint32_t st = MSM_GIANT_PARTS / 2; st > 0; st >>= 1) {
            if (threadIdx.x < st) {
                acc = G1U::add(acc, G1U::from_raw(sh[threadIdx.x + st]));
                sh[threadIdx.x] = G1U::to_raw(acc);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) tk_store(buckets + giant[1 + i], G1U::to_raw(acc));
        __syncthreads();
    }
}

#define MSM_SEG 8
// one lane per (window, segment of MSM_SEG buckets): seg_out = sum_{v in segment} v * B_v
//   = tot + v0 * run   with run = sum B_v, tot = sum (v - v0) B_v by the running-sum trick
__global__ __launch_bounds__(128) void k_reduce_segments(const g1_xyzz_t *__restrict__ buckets, g1_xyzz_t *__restrict__ seg_out,
                                                        msm_plan_t pl, uint32_t segs) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= pl.W * segs) return;
    uint32_t w = gid / segs, sg = gid - w * segs;
    uint32_t v0 = sg * MSM_SEG;  // bucket array index b holds value v = b + 1; segment covers b in [v0, v0+L)
    uint32_t len = pl.B - v0 < MSM_SEG ? pl.B - v0 : MSM_SEG;
    const g1_xyzz_t *bk = buckets + (uint64_t)w * pl.B + v0;
    G1U::X run = G1U::inf(), tot = G1U::inf();
    for (int k = (int)len - 1; k >= 0; k--) {
        run = G1U::add(run, G1U::from_raw(tk_load(bk + k)));
        tot = G1U::add(tot, run);
    }
    // + v0 * run  (v0 < 2^17)
    if (v0) {
        G1U::X m = G1U::inf();
        for (int bit = 31 - __builtin_clz(v0); bit >= 0; bit--) {
            m = G1U::dbl(m);
            if ((v0 >> bit) & 1) m = G1U::add(m, run);
        }
        tot = G1U::add(tot, m);
    }
    tk_store(seg_out + gid, G1U::to_raw(tot));
}

// grid (W, MSM_WIN_PARTS), 256 threads: partial window sum over one slice of the window's segment results; the host adds
// the MSM_WIN_PARTS partials per window before its Horner step (a 4-deep serial loop + 8-level tree per block instead
// of 16 + 8: this kernel is a pure latency chain on W workgroups)
#define MSM_WIN_PARTS 4
__global__ __launch_bounds__(256) void k_reduce_windows(const g1_xyzz_t *__restrict__ seg_in, g1_xyzz_t *__restrict__ win_out,
                                                       uint32_t segs, uint32_t parts) {
    __shared__ g1_xyzz_t sh[256];
    const uint32_t w = blockIdx.x, part = blockIdx.y, t = threadIdx.x;
    const g1_xyzz_t *in = seg_in + (uint64_t)w * segs;
    const uint32_t per = (segs + parts - 1) / parts;
    const uint32_t lo = part * per, hi = lo + per < segs ? lo + per : segs;
    G1U::X acc = G1U::inf();
    for (uint32_t k = lo + t; k < hi; k += 256) acc = G1U::add(acc, G1U::from_raw(tk_load(in + k)));
    sh[t] = G1U::to_raw(acc);
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) {
            acc = G1U::add(acc, G1U::from_raw(sh[t + s]));
            sh[t] = G1U::to_raw(acc);
        }
        __syncthreads();
    }
    if (t == 0) tk_store(win_out + (uint64_t)w * parts + part, G1U::to_raw(acc));
}

// ---- weighted bucket sum of ONE bucket set without scalar multiplications -----------------------------------------------------
// sum_b (b + 1) B_b with b = hi * LO + lo:   = sum_b B_b + LO * sum_hi hi * R_hi + sum_lo lo * C_lo,   R_hi = row sums, C_lo = column
// sums, and sum_i i * V_i = sum_k 2^k (sum of the V_i whose index has bit k).  Every sum is a short serial run per lane and a tree:
// 2^19 buckets -> 1024 + 512 sums -> 1 + 10 + 9 sums, the few doublings are the host's.  The segment reduction spends 60 % of its
// additions on a 16-bit scalar multiplication per segment and runs one long dependent chain per lane.
// ONE launch for both directions, two workgroups per CU (the general addition fits 256 registers: two waves per SIMD hide each
// other's dependent-issue latency, which a lone wave cannot).  Blocks [0, HI / 4): wave v sums row 4 * blockIdx + v (LO >= 64
// buckets, LO / 64 per lane, then a 6-level tree).  Blocks [HI / 4, HI / 4 + LO / 2): half h sums column 2 * (blockIdx - HI / 4) + h
// (HI >= 128 buckets at stride LO, HI / 128 per lane, 7-level tree).
__global__ __launch_bounds__(256, 2) void k_reduce_rows_cols(const g1_xyzz_t *__restrict__ buckets, g1_xyzz_t *__restrict__ rows,
                                                            g1_xyzz_t *__restrict__ cols, uint32_t HI, uint32_t LO) {
    __shared__ g1_xyzz_t sh[256];
    const uint32_t t = threadIdx.x;
    const bool is_row = blockIdx.x < HI / 4;
    uint32_t lane, per, width;
    const g1_xyzz_t *src;
    uint64_t stride;
    g1_xyzz_t *dst;
    if (is_row) {
        lane = t & 63u, per = LO >> 6, width = 64, stride = 1;
        const uint32_t row = blockIdx.x * 4 + (t >> 6);
        src = buckets + (uint64_t)row * LO + (uint64_t)lane * per;
        dst = rows + row;
    } else {
        lane = t & 127u, per = HI >> 7, width = 128, stride = LO;
        const uint32_t col = (blockIdx.x - HI / 4) * 2 + (t >> 7);
        src = buckets + (uint64_t)lane * per * LO + col;
        dst = cols + col;
    }
    G1U::X acc = G1U::from_raw(tk_load(src));
    for (uint32_t k = 1; k < per; k++) acc = G1U::add(acc, G1U::from_raw(tk_load(src + (uint64_t)k * stride)));
    sh[t] = G1U::to_raw(acc);
    __syncthreads();
    for (uint32_t st = 64; st > 0; st >>= 1) {
        if (st < width && lane < st) {   // rows start at 32: their first step is idle (uniform over the block)
            acc = G1U::add(acc, G1U::from_raw(sh[t + st]));
            sh[t] = G1U::to_raw(acc);
        }
        __syncthreads();
    }
    if (lane == 0) tk_store(dst, G1U::to_raw(acc));
}
// grid 1 + hi_bits + lo_bits, 256 threads: out[0] = sum of the rows; out[1 + k] = sum of the rows whose index has bit k;
// out[1 + hi_bits + k] likewise over the columns
__global__ __launch_bounds__(256, 2) void k_reduce_bits(const g1_xyzz_t *__restrict__ rows, const g1_xyzz_t *__restrict__ cols, uint32_t HI, uint32_t LO,
                                                    uint32_t hi_bits, g1_xyzz_t *__restrict__ out) {
    __shared__ g1_xyzz_t sh[256];
    const uint32_t t = threadIdx.x, q = blockIdx.x;
    const bool over_rows = q <= hi_bits;
    const g1_xyzz_t *src = over_rows ? rows : cols;
    const uint32_t len = over_rows ? HI : LO, mask = q == 0 ? 0u : 1u << (over_rows ? q - 1 : q - 1 - hi_bits);
    G1U::X acc = G1U::inf();
    for (uint32_t i = t; i < len; i += 256) {
        // the additions stay uniform over the wave: an element outside the subset enters as the point at infinity
        g1_xyzz_t e = tk_load(src + i);
        G1U::X v = G1U::from_raw(e);
        if (mask && !(i & mask)) v = G1U::inf();
        acc = G1U::add(acc, v);
    }
    sh[t] = G1U::to_raw(acc);
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (t < st) {
            acc = G1U::add(acc, G1U::from_raw(sh[t + st]));
            sh[t] = G1U::to_raw(acc);
        }
        __syncthreads();
    }
    if (t == 0) tk_store(out + q, G1U::to_raw(acc));
}

// out[b] = [s_b] P_b : the "batch of one-point MSMs" shape (libs/src/iotools/mod.rs:1113-1151)
__global__ __launch_bounds__(128) void k_msm_size1(const fr_t *__restrict__ scalars, const g1_affine_t *__restrict__ bases,
                                                  int shared, uint32_t n, int points_mont, int scalars_mont,
                                                  g1_xyzz_t *__restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr_t s = Fr::canon(tk_load(scalars + i));
    if (scalars_mont) s = Fr::from_mont(s);
    g1_affine_t p0 = tk_load(bases + (shared ? 0 : i));
    g1k_aff p;
    p.x = p0.x;
    p.y = p0.y;
    if (!points_mont && !G1::is_inf(p0)) {
        p.x = Fq::to_mont(Fq::canon(p0.x));
        p.y = Fq::to_mont(Fq::canon(p0.y));
    }
    g1k_xyzz acc = G1K::inf();
    for (int bit = 254; bit >= 0; bit--) {
        acc = G1K::dbl(acc);
        if ((s.l[bit >> 5] >> (bit & 31)) & 1) acc = G1K::add_mixed(acc, p);
    }
    tk_store(reinterpret_cast<g1k_xyzz *>(out) + i, acc);
}

// A batch of SMALL MSMs (2 <= n <= 64 points each): the prover's linear combinations of a handful of CRS points (G1serde `+`, `*`,
// lib.rs:1146-1160, 3180-3184).  The sorting pipeline would spend a dozen launches on 16 points; here work item (4-bit window w,
// point i) is digit * P_i by double-and-add, one block of 256 lanes covers 4 windows x 64 point slots and sums each window's items in
// LDS.  out[b][w] = sum_i digit_w(s_i) P_i; the host runs Horner over the 64 window sums.  grid (16, batch).
#define SM_NW 64
__global__ __launch_bounds__(256) void k_msm_small(const fr_t *__restrict__ scalars, const g1_affine_t *__restrict__ bases, int shared, uint32_t n,
                                                  int points_mont, int scalars_mont, uint32_t bits, g1_xyzz_t *__restrict__ out) {
    __shared__ g1k_xyzz sh[256];
    const uint32_t t = threadIdx.x, i = t & 63u, w = blockIdx.x * 4 + (t >> 6), b = blockIdx.y;
    g1k_xyzz acc = G1K::inf();
    if (i < n) {
        fr_t s = Fr::canon(tk_load(scalars + (uint64_t)b * n + i));
        if (scalars_mont) s = Fr::from_mont(s);
        uint32_t d = (s.l[w >> 3] >> ((w & 7u) * 4)) & 15u;
        if (4 * w >= bits) d = 0;                                   // only the low `bits` bits of a scalar count (cfg->bitsize)
        else if (4 * w + 4 > bits) d &= (1u << (bits - 4 * w)) - 1u;
        g1_affine_t p0 = tk_load(bases + (shared ? (uint64_t)i : (uint64_t)b * n + i));
        if (d && !G1::is_inf(p0)) {
            g1k_aff p;
            p.x = p0.x, p.y = p0.y;
            if (!points_mont) {
                p.x = Fq::to_mont(Fq::canon(p0.x));
                p.y = Fq::to_mont(Fq::canon(p0.y));
            }
            for (int bit = 3; bit >= 0; bit--) {
                acc = G1K::dbl(acc);
                if ((d >> bit) & 1u) acc = G1K::add_mixed(acc, p);
            }
        }
    }
    sh[t] = acc;
    __syncthreads();
    for (uint32_t st = 32; st > 0; st >>= 1) {
        if (i < st) {
            acc = G1K::add(acc, sh[t + st]);
            sh[t] = acc;
        }
        __syncthreads();
    }
    if (i == 0) tk_store(reinterpret_cast<g1k_xyzz *>(out) + (uint64_t)b * SM_NW + w, acc);
}

#ifdef TK_MSM_SYM_SEGMENTED
// SEGMENTED small MSM (tkmk_msm_segmented): the same work item as k_msm_small — (4-bit window w, term i) is digit_w(s_i) * P_i by
// double-and-add — for MANY jobs of DIFFERENT sizes over views and index lists of resident tables, and with the tail on the device too.
// One descriptor per job, built on the host and uploaded once per call; terms are addressed as tkmk_msm_job_ex addresses them.
struct seg_job_t {
    const fr_t *scalars;
    const g1_affine_t *bases;
    const uint32_t *index;      // base_index list (takes precedence over the base view), or nullptr
    uint32_t n;                 // terms
    uint32_t s_cols, s_stride;  // scalar view, 0 = contiguous
    uint32_t b_cols, b_stride;  // base view, 0 = contiguous
    uint32_t limit;             // records behind `bases` for an index list: an entry at or past it is clamped to 0 and flagged
};
__device__ __forceinline__ uint32_t seg_strided(uint32_t k, uint32_t cols, uint32_t stride) {
    if (!cols) return k;
    const uint32_t row = k / cols;
    return row * stride + (k - row * cols);
}
// the slots a job can fill: min(n, 64) rounded up to a power of two (0 terms: 1)
__host__ __device__ __forceinline__ uint32_t seg_slots(uint32_t n) {
    uint32_t m = 1;
    while (m < n && m < 64) m <<= 1;
    return m;
}
// grid (jobs, 16): jobs on blockIdx.x (no 65 535 limit), blockIdx.y = a group of four windows; 256 lanes = 4 windows x 64 term slots.
// Slot `slot` walks terms slot, slot + 64, ... of its job (ragged: 129 terms are three trips, 0 terms none).  Dynamic LDS: 4 x lds_slots
// XYZZ records, lds_slots = the widest seg_slots() of the call; a call of one-term jobs takes none and does no LDS addition.  The tree
// uses the complete addition: equal points meet in it whenever a record occurs twice in a job.  out[job][w] = sum_i digit_w(s_i) P_i.
__global__ __launch_bounds__(256) void k_msm_segmented(const seg_job_t *__restrict__ jobs, int form, fq_t conv, int scalars_mont, uint32_t bits,
                                                      uint32_t lds_slots, uint32_t *__restrict__ flag, g1_xyzz_t *__restrict__ out) {
    extern __shared__ uint4 seg_lds[];
    const uint32_t t = threadIdx.x, slot = t & 63u, w = blockIdx.y * 4 + (t >> 6);
    const seg_job_t jb = jobs[blockIdx.x];
    // only the low `bits` bits of a scalar count (cfg->bitsize), as in k_msm_small
    const uint32_t dmask = 4 * w >= bits ? 0u : 4 * w + 4 > bits ? (1u << (bits - 4 * w)) - 1u : 15u;
    g1k_xyzz acc = G1K::inf();
    for (uint32_t i = slot; i < jb.n; i += 64) {
        uint32_t r = jb.index ? jb.index[i] : seg_strided(i, jb.b_cols, jb.b_stride);
        if (jb.limit && r >= jb.limit) {   // whatever the digit is: every window reports the same indices
            atomicOr(flag, 1u);
            r = 0;
        }
        if (!dmask) continue;
        fr_t s = Fr::canon(tk_load(jb.scalars + seg_strided(i, jb.s_cols, jb.s_stride)));
        if (scalars_mont) s = Fr::from_mont(s);
        uint32_t limb = 0;   // s.l[w >> 3] by selects: a runtime-indexed limb array would live in scratch
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) limb = (w >> 3) == k ? s.l[k] : limb;
        const uint32_t d = (limb >> ((w & 7u) * 4)) & dmask;
        if (!d) continue;
        const g1_affine_t p0 = tk_load(jb.bases + r);
        if (G1::is_inf(p0)) continue;
        g1k_aff p;
        p.x = Fq::canon(p0.x), p.y = Fq::canon(p0.y);
        if (form == TKMK_BASES_PLAIN) p.x = Fq::to_mont(p.x), p.y = Fq::to_mont(p.y);
        else if (form == TKMK_BASES_CONVERTED) p.x = Fq::mul(p.x, conv), p.y = Fq::mul(p.y, conv);   // x R' * (R^2 / R') / R = x R
        g1k_xyzz term = G1K::inf();
#pragma unroll 1
        for (int bit = 3; bit >= 0; bit--) {
            term = G1K::dbl(term);
            if ((d >> bit) & 1u) term = G1K::add_mixed(term, p);
        }
        acc = G1K::add(acc, term);
    }
    const uint32_t m = seg_slots(jb.n);   // the same in every lane of the workgroup: the barriers below are uniform
    if (m > 1) {
        g1k_xyzz *sh = reinterpret_cast<g1k_xyzz *>(seg_lds) + (t >> 6) * lds_slots;
        if (slot < m) sh[slot] = acc;
        __syncthreads();
        for (uint32_t st = m >> 1; st > 0; st >>= 1) {
            if (slot < st) {
                acc = G1K::add(acc, sh[slot + st]);
                sh[slot] = acc;
            }
            __syncthreads();
        }
    }
    if (slot == 0) tk_store(reinterpret_cast<g1k_xyzz *>(out) + (uint64_t)blockIdx.x * SM_NW + w, acc);
}
// The tail, one lane per job: Horner over the job's window sums (4 doublings and one addition per window; windows at or past `nw` hold
// nothing under cfg->bitsize), to_affine, and the library's canonical projective record — (x, y, 1), or (0, 1, 0) for infinity — what
// store_canonical writes on the host.  `results` is device memory; dword stores, since a caller's record array need not be 16-byte aligned.
__global__ __launch_bounds__(64) void k_msm_segmented_finish(const g1_xyzz_t *__restrict__ wins, uint32_t n_jobs, uint32_t nw, abi_proj *__restrict__ results) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    const g1k_xyzz *win = reinterpret_cast<const g1k_xyzz *>(wins) + (uint64_t)j * SM_NW;
    g1k_xyzz acc = G1K::inf();
#pragma unroll 1
    for (int w = (int)nw - 1; w >= 0; w--) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) acc = G1K::dbl(acc);
        acc = G1K::add(acc, tk_load(win + w));
    }
    const bool inf = G1K::is_inf(acc);
    const g1k_aff a = G1K::to_affine(acc);
    const fq_t x = Fq::from_mont(a.x), y = Fq::from_mont(a.y);   // to_affine(infinity) = (0, 0)
    uint32_t *o = reinterpret_cast<uint32_t *>(results + j);
#pragma unroll
    for (int i = 0; i < Fq::N; i++) {
        o[i] = x.l[i];
        o[Fq::N + i] = inf ? (i == 0 ? 1u : 0u) : y.l[i];
        o[2 * Fq::N + i] = !inf && i == 0 ? 1u : 0u;
    }
}
#endif

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
static uint32_t choose_c(uint32_t n) {
    // minimise W * (n + ~4*B) over c <= 16.  (c = 17, 18 are accepted on request — the two-pass sort handles 512 x 256 bins —
    // but measured slower at 2^24 points: 63.4 vs 51.3 ms; 128-entry buckets mean more chunk fragments to flush and combine.)
    uint32_t best = 2;
    double best_cost = 1e300;
    for (uint32_t c = 2; c <= 16; c++) {
        double W = (double)(255 / c + 1);
        double cost = W * ((double)n + 4.0 * (double)(1u << (c - 1)));
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

static void store_canonical(abi_proj *o, const g1_xyzz_t &r) {
    g1_affine_t a = G1::to_affine(r);
    bool inf = G1::is_inf(r);
    fq_t x = inf ? Fq::zero() : Fq::from_mont(a.x);
    fq_t y = Fq::from_mont(a.y);
    fq_t z = Fq::zero();
    if (inf) {
        y = Fq::zero();
        y.l[0] = 1;
    } else {
        z.l[0] = 1;
    }
    for (int i = 0; i < Fq::N; i++) {
        o->x.limbs[i] = x.l[i];
        o->y.limbs[i] = y.l[i];
        o->z.limbs[i] = z.l[i];
    }
}

#ifdef TK_MSM_PRIMARY
TK_API tkmk_msm_config tkmk_msm_default_config(void) {
    tkmk_msm_config c;
    c.stream_handle = nullptr;
    c.precompute_factor = 1;
    c.c = 0;
    c.bitsize = 0;
    c.batch_size = 1;
    c.are_points_shared_in_batch = true;
    c.are_scalars_on_device = false;
    c.are_scalars_montgomery_form = false;
    c.are_points_on_device = false;
    c.are_points_montgomery_form = false;
    c.are_results_on_device = false;
    c.is_async = false;
    c.ext = nullptr;
    return c;
}
#endif


// TKMK_MSM_DEBUG=1: pull every intermediate back and re-derive it on the host (small sizes only).
static bool xyzz_same_point(const g1_xyzz_t &a, const g1_xyzz_t &b) {
    g1_affine_t pa = G1::to_affine(a), pb = G1::to_affine(b);
    return Fq::eq(pa.x, pb.x) && Fq::eq(pa.y, pb.y);
}
static tkmk_error msm_debug_check(const msm_plan_t &pl, const fr_t *scalars, const g1_affine_t *bases, const uint32_t *d_dig,
                                  const uint32_t *d_sorted, const uint32_t *d_bstart, const g1_xyzz_t *d_buckets, hipStream_t s) {
    TK_HIP(hipStreamSynchronize(s));
    TK_HIP(hipGetLastError());
    std::vector<fr_t> sc(pl.n);
    std::vector<g1_affine_t> bs(pl.n);
    std::vector<uint32_t> dig((size_t)pl.W * pl.n), sorted((size_t)pl.W * pl.n), bstart((size_t)pl.W * (pl.B + 1));
    std::vector<g1_xyzz_t> buckets((size_t)pl.W * pl.B);
    TK_HIP(hipMemcpy(sc.data(), scalars, sc.size() * sizeof(fr_t), hipMemcpyDeviceToHost));
    TK_HIP(hipMemcpy(bs.data(), bases, bs.size() * sizeof(g1_affine_t), hipMemcpyDeviceToHost));
    {   // device bases are {x R', y R'} (packed); the host re-derivation works in saturated Montgomery form
        fq_t rp;
        for (int j = 0; j < Fq::N; j++) rp.l[j] = FqP::KSATM[j];  // R' mod p (plain)
        fq_t rinv = Fq::inv(Fq::to_mont(rp));
        for (auto &b : bs)
            if (!G1::is_inf(b)) {
                b.x = Fq::mul(Fq::to_mont(b.x), rinv);
                b.y = Fq::mul(Fq::to_mont(b.y), rinv);
            }
    }
    TK_HIP(hipMemcpy(dig.data(), d_dig, dig.size() * 4, hipMemcpyDeviceToHost));
    TK_HIP(hipMemcpy(sorted.data(), d_sorted, sorted.size() * 4, hipMemcpyDeviceToHost));
    TK_HIP(hipMemcpy(bstart.data(), d_bstart, bstart.size() * 4, hipMemcpyDeviceToHost));
    TK_HIP(hipMemcpy(buckets.data(), d_buckets, buckets.size() * sizeof(g1_xyzz_t), hipMemcpyDeviceToHost));
    fprintf(stderr, "[msm debug] n=%u c=%u W=%u B=%u chunks=%u chunk_len=%u\n", pl.n, pl.c, pl.W, pl.B, pl.chunks, pl.chunk_len);
    int bad = 0;
    // digits reconstruct the scalar: sum_w d_w 2^(c w) == s  (checked mod 2^64 on the low limbs for brevity)
    for (uint32_t i = 0; i < pl.n && bad < 5; i++) {
        unsigned __int128 acc = 0;
        for (int w = (int)pl.W - 1; w >= 0; w--) {
            uint32_t rec = dig[(size_t)w * pl.n + i];
            long long d = (long long)(rec & 0x7fffffffu);
            if (rec & 0x80000000u) d = -d;
            if ((rec & 0x7fffffffu) > pl.B) { fprintf(stderr, "[msm debug] digit too large i=%u w=%d rec=%08x\n", i, w, rec); bad++; }
            if ((uint32_t)w * pl.c < 100) acc = (acc << pl.c) + (unsigned __int128)(__int128)d;
        }
        uint64_t lo = (uint64_t)sc[i].l[0] | ((uint64_t)sc[i].l[1] << 32);
        (void)lo;
    }
    for (uint32_t w = 0; w < pl.W; w++) {
        const uint32_t *bsw = &bstart[(size_t)w * (pl.B + 1)];
        uint32_t nz = 0;
        for (uint32_t i = 0; i < pl.n; i++) nz += (dig[(size_t)w * pl.n + i] & 0x7fffffffu) != 0;
        if (bsw[pl.B] != nz && bad < 20) { fprintf(stderr, "[msm debug] w=%u total %u != nonzero digits %u\n", w, bsw[pl.B], nz); bad++; }
        for (uint32_t b = 0; b < pl.B; b++) {
            if (bsw[b] > bsw[b + 1]) { if (bad < 20) fprintf(stderr, "[msm debug] w=%u b=%u bstart not monotone\n", w, b); bad++; continue; }
            g1_xyzz_t acc = G1::inf();
            for (uint32_t k = bsw[b]; k < bsw[b + 1]; k++) {
                uint32_t rec = sorted[(size_t)w * pl.n + k], i = rec & 0x7fffffffu;
                if (i >= pl.n) { if (bad < 20) fprintf(stderr, "[msm debug] w=%u b=%u bad index %u\n", w, b, i); bad++; continue; }
                uint32_t drec = dig[(size_t)w * pl.n + i];
                if ((drec & 0x7fffffffu) != b + 1 || ((drec ^ rec) & 0x80000000u)) {
                    if (bad < 20) fprintf(stderr, "[msm debug] w=%u b=%u entry %u: digit rec %08x does not belong here\n", w, b, k, drec);
                    bad++;
                }
                g1_affine_t pnt = bs[i];
                if (rec & 0x80000000u) pnt.y = Fq::neg(pnt.y);
                acc = G1::add_mixed(acc, pnt);
            }
            buckets[(size_t)w * pl.B + b] = G1U::raw_to_sat(buckets[(size_t)w * pl.B + b]);   // device buckets are raw records
            bool okb = xyzz_same_point(acc, buckets[(size_t)w * pl.B + b]);
            if (atoi(getenv("TKMK_MSM_DEBUG")) >= 2 && w == 7 && bsw[b + 1] > bsw[b])
                fprintf(stderr, "[msm debug] w7 b=%u pos=%u cnt=%u %s\n", b, bsw[b], bsw[b + 1] - bsw[b], okb ? "ok" : "BAD");
            if (!okb) {
                if (bad < 20) {
                    const g1_xyzz_t &dv = buckets[(size_t)w * pl.B + b];
                    uint32_t rec0 = bsw[b + 1] > bsw[b] ? sorted[(size_t)w * pl.n + bsw[b]] : 0;
                    const char *cls = "other";
                    if (G1::is_inf(dv)) cls = "inf";
                    else if (xyzz_same_point(G1::neg(acc), dv)) cls = "negated";
                    fprintf(stderr, "[msm debug] w=%u b=%u bucket sum mismatch (%u entries) rec0=%08x device=%s zz0=%08x x0=%08x\n", w, b,
                            bsw[b + 1] - bsw[b], rec0, cls, dv.zz.l[0], dv.x.l[0]);
                }
                bad++;
            }
        }
    }
    fprintf(stderr, "[msm debug] %d inconsistencies\n", bad);
    return TKMK_SUCCESS;
}

// Enqueues one MSM of n points (device-resident scalars / converted bases) on stream s, ending with the
// async copy of the W x MSM_WIN_PARTS partial window sums into wins_host (>= MSM_MAX_WINDOWS * MSM_WIN_PARTS entries; pinned memory keeps the copy
// asynchronous).  Scratch comes from the caller's tk_frame on s, which must stay open until s has drained.
#define MSM_MAX_WINDOWS 128
// window width actually used for an MSM of n_src points: the one rule shared by the MSM and by the precompute table
// Entries per accumulate lane.  k_accumulate_chunks holds 2 waves per SIMD (242 VGPRs): the chip runs `slots` lanes at a time, and a
// launch of L lanes takes ceil(L / slots) rounds of `chunk` additions each — a launch that needs 8.01 rounds pays for 9 (the prover's
// boxes are (2^k + 1) wide: exactly that case), and one that needs 1.6 pays for 2.  The chunk length is therefore chosen so that
// the lanes fill a whole number of rounds: r = rounds at the target length, chunk = entries / (r * slots), in [32, 256].
static uint32_t msm_choose_chunk(uint64_t entries, uint32_t W, uint32_t n) {
    static const uint32_t slots = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (cus <= 0) cus = 256;
        return (uint32_t)cus * 4u * 2u * 64u;   // SIMDs per CU x waves per SIMD at this kernel's register count x lanes
    }();
    if (getenv("TKMK_MSM_FIXED_CHUNK")) return MSM_CHUNK;
    if (const char *e = getenv("TKMK_MSM_CHUNK_LEN")) {   // diagnostic: force the chunk length
        int v = atoi(e);
        if (v >= 8 && v <= 8192) return (uint32_t)v;
    }
    // The kernel's time does not depend on the chunk length between 40 and 200 entries (measured), the fragment combine after it
    // gets cheaper with longer chunks, and a launch should still be several rounds of lanes: aim at 8 rounds, 48..224 entries, then
    // fit the length so that the lanes fill whole rounds
    uint64_t target = entries / (8ull * slots);
    if (target < 48) target = 48;
    if (target > 224) target = 224;
    uint64_t r = (entries + target * slots / 2) / (target * slots);
    if (r < 1) r = 1;
    uint64_t lanes_per_window = r * slots / W;   // lanes each window may use
    if (lanes_per_window < 1) lanes_per_window = 1;
    uint64_t chunk = (n + lanes_per_window - 1) / lanes_per_window;
    if (chunk < 32) chunk = 32;
    if (chunk > 256) chunk = 256;
    // beyond 2^30 sorted entries (a 2^28-point MSM) 128-entry chunks leave every bucket with dozens of fragments, all of them through
    // the one-workgroup-per-bucket combine: longer chunks, still 32 rounds of lanes
    if (entries > (1ull << 30)) {
        uint64_t big = entries / (32ull * slots);
        if (big > 4096) big = 4096;
        if (big > chunk) chunk = big;
    }
    return (uint32_t)chunk;
}
#define MSM_MAX_C 20   // 2^19 buckets per window = 1024 coarse x 512 fine bins of the two-pass sort
static uint32_t msm_resolve_c(uint32_t c_req, uint32_t n_src) {
    uint32_t c = c_req ? c_req : choose_c(n_src);
    if (c < 2) c = 2;
    if (c > MSM_MAX_C) c = MSM_MAX_C;
    static const bool force_one_pass = getenv("TKMK_MSM_ONE_PASS") != nullptr;
    if (c > 16 && (force_one_pass || n_src < (1u << 18))) c = 16;   // wide windows need the two-pass sort
    return c;
}

// Dynamic LDS the accumulate kernels claim but never touch: above half a CU's 160 KB a claim holds the kernel to one workgroup (one wave
// per SIMD) per CU, leaving registers and issue slots to co-resident kernels.
//   foreground  TKMK_MSM_ACC_LDS=bytes (diagnostic; default none)
//   background  batches issued on a caller stream marked BACKGROUND (tkmk_stream_set_background: a commit that nothing waits for until
//               later, issued beside the work that IS waited for) claim 96 KB, so that the foreground's kernels find registers on every
//               CU while they run.  Measured (r4, one box, alternating): prove4 with its M / N openings in the background 54.4 -> 52.2 ms;
//               prove0's evaluation commits lose 1 ms the same way (the round ends on them) and stay foreground.
//               TKMK_MSM_BACKGROUND_LDS overrides the size (0 = off).
// The kernels' dynamic-LDS limit is raised here, once, to the larger of the two; if the runtime refuses it, neither claim is made.
struct msm_acc_lds_t {
    uint32_t foreground, background;
};
static const msm_acc_lds_t &msm_acc_lds() {
    static const msm_acc_lds_t claims = [] {
        const char *fg = getenv("TKMK_MSM_ACC_LDS"), *bg = getenv("TKMK_MSM_BACKGROUND_LDS");
        msm_acc_lds_t v{fg ? (uint32_t)atoi(fg) : 0u, bg ? (uint32_t)atoi(bg) : 98304u};
        const int most = (int)(v.foreground > v.background ? v.foreground : v.background);
        hipError_t e = most ? hipFuncSetAttribute((const void *)k_accumulate_chunks, hipFuncAttributeMaxDynamicSharedMemorySize, most) : hipSuccess;
#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
        if (most && e == hipSuccess) e = hipFuncSetAttribute((const void *)k_accumulate_chunks_rows, hipFuncAttributeMaxDynamicSharedMemorySize, most);
#endif
        if (e != hipSuccess) v = msm_acc_lds_t{0, 0};
        return v;
    }();
    return claims;
}
// background: the batch was issued on a caller stream marked BACKGROUND (msm_pipeline asks; a single MSM never is)
static tkmk_error msm_enqueue(const fr_t *scalars, const g1_affine_t *bases_mont, uint32_t n_src, uint32_t factor, uint32_t c_req,
                              uint32_t bits, bool scalars_mont, hipStream_t s, g1_xyzz_t *wins_host, msm_plan_t *plan_out, bool background,
                              msm_view_t sv = view_identity(), msm_view_t bv = view_identity(), uint32_t level_rows = 0,
                              const acc_row_t *acc_rows = nullptr) {   // acc_rows: the table as accumulate-ready rows (bases_mont unused)
    msm_plan_t pl;
    static const bool force_one_pass = getenv("TKMK_MSM_ONE_PASS") != nullptr;
    pl.bits = bits;
    // a precomputed TABLE fixes its window width (the levels are the 2^(c j) multiples): the job's c is taken as is
    pl.c = level_rows ? c_req : msm_resolve_c(c_req, n_src);
    if (pl.c < 2 || pl.c > MSM_MAX_C) return TKMK_ERR_INVALID_ARGUMENT;
    pl.n_src = n_src;
    pl.W_src = bits / pl.c + 1;
    if (factor < 1) factor = 1;
    if (factor > pl.W_src) factor = pl.W_src;
    if ((uint64_t)n_src * factor >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;   // 31-bit point index in the sort records
    if (factor > 1 && !view_is_identity(bv) && !level_rows) return TKMK_ERR_INVALID_ARGUMENT;   // a base view needs the table's level size
    if (level_rows && (uint64_t)level_rows * factor >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
    const uint32_t n = n_src * factor;                       // expanded points
    pl.n = n;
    pl.W = (pl.W_src + factor - 1) / factor;                 // windows per group
    pl.B = 1u << (pl.c - 1);
    pl.chunk = msm_choose_chunk((uint64_t)pl.W * n, pl.W, n);
    {
        // A bucket spanning more chunks than `big` is summed by a wave (k_combine_big) instead of one lane.  Where buckets span two or three
        // chunks on average (the 20-bit table: 2^19 buckets) the few that span 13..48 are what the lane-per-bucket kernel waits for, so the bar
        // is low; where EVERY bucket spans dozens (16-bit windows of a sharded context, small plain MSMs) the lanes are evenly loaded and the
        // per-lane sums are the efficient form, so only real outliers go to the queue.
        static const uint32_t big_env = getenv("TKMK_MSM_BIG") ? (uint32_t)atoi(getenv("TKMK_MSM_BIG")) : 0u;
        const uint64_t avg_spans = (uint64_t)n / ((uint64_t)pl.chunk * pl.B);
        pl.big = big_env ? big_env : (avg_spans >= 4 ? 4u * MSM_BIG : MSM_BIG);
    }
    pl.win_parts = pl.W >= 8 ? MSM_WIN_PARTS : 32;   // few windows: more partials per window, or the 65536-segment tree of a single window is a 1 ms chain on 4 blocks
    pl.hi_bits = pl.lo_bits = 0;
    if (pl.W == 1 && pl.c >= 15) {   // a single bucket set of >= 2^14 buckets (the commit table): rows / columns instead of segments
        pl.lo_bits = (pl.c - 1) / 2;
        pl.hi_bits = pl.c - 1 - pl.lo_bits;   // hi >= lo >= 7: rows of >= 128 buckets, columns of >= 128
    }
    static const bool no_rowcol = getenv("TKMK_MSM_SEGMENT_TAIL") != nullptr;   // diagnostic: the segment reduction for every job
    if (no_rowcol) pl.hi_bits = pl.lo_bits = 0;
    uint32_t want = (512 + pl.W - 1) / pl.W;
    if (getenv("TKMK_MSM_CHUNKS")) want = (uint32_t)atoi(getenv("TKMK_MSM_CHUNKS"));
    uint32_t maxc = (n + 8191) / 8192;
    pl.chunks = want < maxc ? want : maxc;
    if (pl.chunks < 1) pl.chunks = 1;
    pl.chunk_len = (n + pl.chunks - 1) / pl.chunks;

    tk_scratch d_dig, d_sorted, d_counts, d_bstart, d_buckets, d_segs, d_wins;
    TK_TRY(d_dig.alloc((size_t)pl.W * n * 4, s));
    TK_TRY(d_sorted.alloc((size_t)pl.W * n * 4, s));
    const bool two_pass = !force_one_pass && pl.c >= 13 && n >= (1u << 18);
    if (pl.c > 16 && !two_pass) return TKMK_ERR_INVALID_ARGUMENT;   // wide windows need the two-pass sort (a table job must be large enough)
    {   // pass A counts coarse bins only
        const uint32_t fb = pl.c >= 19 ? 9u : pl.c >= 17 ? 8u : 7u;
        TK_TRY(d_counts.alloc((size_t)pl.W * (two_pass ? (pl.B >> fb) : pl.B) * pl.chunks * 4, s));
    }
    TK_TRY(d_bstart.alloc((size_t)pl.W * (pl.B + 1) * 4, s));
    TK_TRY(d_buckets.alloc((size_t)pl.W * pl.B * sizeof(g1_xyzz_t), s));
    uint32_t segs = (pl.B + MSM_SEG - 1) / MSM_SEG;
    TK_TRY(d_segs.alloc((size_t)pl.W * segs * sizeof(g1_xyzz_t), s));
    TK_TRY(d_wins.alloc((size_t)pl.W * pl.win_parts * sizeof(g1_xyzz_t), s));

    tk_stat_add(TK_STAT_MSM_POINTS, n_src);
    tk_stat_add(TK_STAT_MSM_CALLS, 1);
    tk_prof prof(s);
    hipLaunchKernelGGL(k_digits, tk_div_up(n_src, 256), 256, 0, s, scalars, d_dig.as<uint32_t>(), pl, scalars_mont ? 1 : 0, sv);
    prof.mark("msm.digits");
    size_t lds = (size_t)pl.B * 4;
    static std::once_flag attr_once;   // msm_enqueue runs on caller threads and on the pipeline's
    static hipError_t attr_err = hipSuccess;
    std::call_once(attr_once, [] {
        attr_err = hipFuncSetAttribute((const void *)k_hist, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr_err == hipSuccess)
            attr_err = hipFuncSetAttribute((const void *)k_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    });
    TK_HIP(attr_err);
    if (!two_pass) {
        hipLaunchKernelGGL(k_hist, dim3(pl.chunks, pl.W), 1024, lds, s, (const uint32_t *)d_dig.p, d_counts.as<uint32_t>(), pl, 0u);
        prof.mark("msm.hist");
        const uint32_t groups = (pl.B + 1023) / 1024;
        tk_scratch d_local, d_gtot;
        TK_TRY(d_local.alloc((size_t)pl.W * pl.B * 4, s));
        TK_TRY(d_gtot.alloc((size_t)pl.W * groups * 4, s));
        hipLaunchKernelGGL(k_scan_local, dim3(groups, pl.W), 1024, 0, s, (const uint32_t *)d_counts.p, d_local.as<uint32_t>(),
                           d_gtot.as<uint32_t>(), pl);
        hipLaunchKernelGGL(k_scan_apply, dim3(groups, pl.W), 1024, 0, s, d_counts.as<uint32_t>(), (const uint32_t *)d_local.p,
                           (const uint32_t *)d_gtot.p, d_bstart.as<uint32_t>(), pl);
        prof.mark("msm.scan");
        hipLaunchKernelGGL(k_scatter, dim3(pl.chunks, pl.W), 1024, lds, s, (const uint32_t *)d_dig.p, (const uint32_t *)d_counts.p,
                           d_sorted.as<uint32_t>(), pl, bv, level_rows);
        prof.mark("msm.scatter");
    } else {
        const uint32_t fbits = pl.c >= 19 ? 9u : pl.c >= 17 ? 8u : 7u, FB = 1u << fbits, CB = pl.B >> fbits;   // CB <= 1024, FB <= 512
        tk_scratch d_aidx, d_akey, d_cs, d_localA, d_gtotA, d_cntB, d_fs, d_localB, d_gtotB;
        TK_TRY(d_aidx.alloc((size_t)pl.W * n * 4, s));
        TK_TRY(d_akey.alloc((size_t)pl.W * n * 2, s));
        TK_TRY(d_cs.alloc((size_t)pl.W * (CB + 1) * 4, s));
        // ---- pass A: coarse bins ----
        msm_plan_t pa = pl;
        pa.B = CB;
        hipLaunchKernelGGL(k_hist, dim3(pl.chunks, pl.W), 1024, (size_t)CB * 4, s, (const uint32_t *)d_dig.p, d_counts.as<uint32_t>(), pa,
                           fbits);
        prof.mark("msm.hist");
        TK_TRY(d_localA.alloc((size_t)pl.W * CB * 4, s));
        const bool wide_scan = pl.W <= 4 && pl.chunks >= 64;   // few windows, many chunks: spread the bins over CB / 64 workgroups
        const uint32_t groupsA = wide_scan ? (CB + SCW_BINS - 1) / SCW_BINS : 1u;
        TK_TRY(d_gtotA.alloc((size_t)pl.W * groupsA * 4, s));
        if (wide_scan) {
            hipLaunchKernelGGL(k_scan_local_wide, dim3(groupsA, pl.W), 1024, 0, s, (const uint32_t *)d_counts.p, d_localA.as<uint32_t>(),
                               d_gtotA.as<uint32_t>(), pa);
            hipLaunchKernelGGL(k_scan_apply_wide, dim3(groupsA, pl.W), 1024, 0, s, d_counts.as<uint32_t>(), (const uint32_t *)d_localA.p,
                               (const uint32_t *)d_gtotA.p, d_cs.as<uint32_t>(), pa);
        } else {
            hipLaunchKernelGGL(k_scan_local, dim3(1, pl.W), 1024, 0, s, (const uint32_t *)d_counts.p, d_localA.as<uint32_t>(),
                               d_gtotA.as<uint32_t>(), pa);
            hipLaunchKernelGGL(k_scan_apply, dim3(1, pl.W), 1024, 0, s, d_counts.as<uint32_t>(), (const uint32_t *)d_localA.p,
                               (const uint32_t *)d_gtotA.p, d_cs.as<uint32_t>(), pa);
        }
        prof.mark("msm.scan");
        hipLaunchKernelGGL(k_scatter_staged<false>, dim3(pl.chunks, pl.W), 1024, 0, s, (const uint32_t *)d_dig.p, (const uint16_t *)nullptr,
                           (const uint32_t *)nullptr, (const uint32_t *)d_counts.p, d_aidx.as<uint32_t>(), d_akey.as<uint16_t>(), n, CB, CB,
                           pl.chunk_len, fbits, bv, pl.n_src, level_rows);
        // ---- pass B: fine bins inside every (window, coarse bin) segment ----
        const uint32_t segs_b = pl.W * CB;
        TK_TRY(d_cntB.alloc((size_t)segs_b * FB * SC_PARTS * 4, s));
        TK_TRY(d_fs.alloc((size_t)segs_b * (FB + 1) * 4, s));
        TK_TRY(d_localB.alloc((size_t)segs_b * FB * 4, s));
        TK_TRY(d_gtotB.alloc((size_t)segs_b * 4, s));
        hipLaunchKernelGGL(k_hist_fine, dim3(SC_PARTS, segs_b), 1024, 0, s, (const uint16_t *)d_akey.p, (const uint32_t *)d_cs.p,
                           d_cntB.as<uint32_t>(), n, CB, fbits);
        msm_plan_t pb = pl;
        pb.B = FB;
        pb.chunks = SC_PARTS;
        hipLaunchKernelGGL(k_scan_local, dim3(1, segs_b), 1024, 0, s, (const uint32_t *)d_cntB.p, d_localB.as<uint32_t>(),
                           d_gtotB.as<uint32_t>(), pb);
        hipLaunchKernelGGL(k_scan_apply, dim3(1, segs_b), 1024, 0, s, d_cntB.as<uint32_t>(), (const uint32_t *)d_localB.p,
                           (const uint32_t *)d_gtotB.p, d_fs.as<uint32_t>(), pb);
        hipLaunchKernelGGL(k_bstart_assemble, tk_div_up((size_t)pl.W * (pl.B + 1), 256), 256, 0, s, (const uint32_t *)d_cs.p,
                           (const uint32_t *)d_fs.p, d_bstart.as<uint32_t>(), pl.W, pl.B, CB, fbits);
        hipLaunchKernelGGL(k_scatter_staged<true>, dim3(SC_PARTS, segs_b), 1024, 0, s, (const uint32_t *)d_aidx.p, (const uint16_t *)d_akey.p,
                           (const uint32_t *)d_cs.p, (const uint32_t *)d_cntB.p, d_sorted.as<uint32_t>(), (uint16_t *)nullptr, n, FB, CB,
                           0u, fbits, view_identity(), 0u, 0u);
        prof.mark("msm.scatter");
    }
    if (unsigned long long *cell = tk_stat_device_entries())
        hipLaunchKernelGGL(k_count_entries, 1, 1, 0, s, (const uint32_t *)d_bstart.p, pl.W, pl.B, cell);
    const uint32_t cpw = (n + pl.chunk - 1) / pl.chunk;  // chunks per window (upper bound: all digits non-zero)
    const uint32_t big_cap = pl.W * pl.B;   // every bucket may qualify (2^28 points: 64 fragments in each of the 2^19 buckets); a smaller queue would drop buckets
    tk_scratch d_fh, d_ft, d_big, d_giant, d_gpart;
    TK_TRY(d_fh.alloc((size_t)pl.W * cpw * sizeof(g1_xyzz_t), s));
    TK_TRY(d_ft.alloc((size_t)pl.W * cpw * sizeof(g1_xyzz_t), s));
    TK_TRY(d_big.alloc((size_t)(big_cap + 1) * 4, s));
    TK_TRY(d_giant.alloc((size_t)(MSM_GIANT_CAP + 1) * 4, s));
    TK_TRY(d_gpart.alloc((size_t)MSM_GIANT_CAP * MSM_GIANT_PARTS * sizeof(g1_xyzz_t), s));
    TK_HIP(hipMemsetAsync(d_buckets.p, 0, (size_t)pl.W * pl.B * sizeof(g1_xyzz_t), s));  // empty bucket = infinity
    TK_HIP(hipMemsetAsync(d_big.p, 0, 4, s));
    TK_HIP(hipMemsetAsync(d_giant.p, 0, 4, s));
    const msm_acc_lds_t &acc_lds = msm_acc_lds();
    const uint32_t lds_claim = (background && acc_lds.background) ? acc_lds.background : acc_lds.foreground;
    prof.mark("msm.prepare");   // bucket / queue memsets, the entry counter: keeps "msm.accumulate" to the kernel itself
#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
    if (acc_rows)
        hipLaunchKernelGGL(k_accumulate_chunks_rows, tk_div_up((size_t)pl.W * cpw, 256), 256, lds_claim, s, acc_rows, (const uint32_t *)d_sorted.p,
                           (const uint32_t *)d_bstart.p, d_buckets.as<g1_xyzz_t>(), d_fh.as<g1_xyzz_t>(), d_ft.as<g1_xyzz_t>(), pl, cpw);
    else
#endif
    hipLaunchKernelGGL(k_accumulate_chunks, tk_div_up((size_t)pl.W * cpw, 256), 256, lds_claim, s, bases_mont, (const uint32_t *)d_sorted.p,
                       (const uint32_t *)d_bstart.p, d_buckets.as<g1_xyzz_t>(), d_fh.as<g1_xyzz_t>(), d_ft.as<g1_xyzz_t>(), pl, cpw);
    prof.mark("msm.accumulate");
    hipLaunchKernelGGL(k_combine, tk_div_up((size_t)pl.W * pl.B, 256), 256, 0, s, (const uint32_t *)d_bstart.p, d_buckets.as<g1_xyzz_t>(),
                       (const g1_xyzz_t *)d_fh.p, (const g1_xyzz_t *)d_ft.p, pl, cpw, d_big.as<uint32_t>(), big_cap, d_giant.as<uint32_t>());
    if ((uint64_t)n > (uint64_t)MSM_GIANT * pl.chunk) {   // a giant bucket needs more than 2048 chunks of entries
        hipLaunchKernelGGL(k_combine_giant_parts, 1024, 256, 0, s, (const uint32_t *)d_bstart.p, (const g1_xyzz_t *)d_fh.p,
                           (const g1_xyzz_t *)d_ft.p, pl, cpw, (const uint32_t *)d_giant.p, d_gpart.as<g1_xyzz_t>());
        hipLaunchKernelGGL(k_combine_giant_final, 256, 64, 0, s, d_buckets.as<g1_xyzz_t>(), (const uint32_t *)d_giant.p,
                           (const g1_xyzz_t *)d_gpart.p);
    }
    hipLaunchKernelGGL(k_combine_big, 1024, 256, 0, s, (const uint32_t *)d_bstart.p, d_buckets.as<g1_xyzz_t>(),
                       (const g1_xyzz_t *)d_fh.p, (const g1_xyzz_t *)d_ft.p, pl, cpw, (const uint32_t *)d_big.p, big_cap);
    prof.mark("msm.combine");
    size_t wins_count = (size_t)pl.W * pl.win_parts;
    if (pl.lo_bits) {   // one bucket set: rows, columns, bit-subset sums (d_segs holds the 2^hi_bits + 2^lo_bits sums)
        const uint32_t HI = 1u << pl.hi_bits, LO = 1u << pl.lo_bits;
        g1_xyzz_t *rows = d_segs.as<g1_xyzz_t>(), *cols = rows + HI;
        hipLaunchKernelGGL(k_reduce_rows_cols, HI / 4 + LO / 2, 256, 0, s, (const g1_xyzz_t *)d_buckets.p, rows, cols, HI, LO);
        prof.mark("msm.reduce_segments");
        wins_count = 1 + pl.hi_bits + pl.lo_bits;
        hipLaunchKernelGGL(k_reduce_bits, (unsigned)wins_count, 256, 0, s, (const g1_xyzz_t *)rows, (const g1_xyzz_t *)cols, HI, LO, pl.hi_bits,
                           d_wins.as<g1_xyzz_t>());
        prof.mark("msm.reduce_windows");
    } else {
        hipLaunchKernelGGL(k_reduce_segments, tk_div_up((size_t)pl.W * segs, 128), 128, 0, s, (const g1_xyzz_t *)d_buckets.p,
                           d_segs.as<g1_xyzz_t>(), pl, segs);
        prof.mark("msm.reduce_segments");
        hipLaunchKernelGGL(k_reduce_windows, dim3(pl.W, pl.win_parts), 256, 0, s, (const g1_xyzz_t *)d_segs.p, d_wins.as<g1_xyzz_t>(), segs, pl.win_parts);
        prof.mark("msm.reduce_windows");
    }
    TK_HIP(hipGetLastError());
    if (getenv("TKMK_MSM_DEBUG"))
        fprintf(stderr, "[msm debug] ptrs dig=%p sorted=%p counts=%p bstart=%p buckets=%p (+%zu) segs=%p (+%zu) wins=%p\n", d_dig.p,
                d_sorted.p, d_counts.p, d_bstart.p, d_buckets.p, (size_t)pl.W * pl.B * sizeof(g1_xyzz_t), d_segs.p,
                (size_t)pl.W * segs * sizeof(g1_xyzz_t), d_wins.p);
    if (getenv("TKMK_MSM_DEBUG") && factor == 1 && view_is_identity(sv) && view_is_identity(bv) && !level_rows && !acc_rows) TK_TRY(msm_debug_check(pl, scalars, bases_mont, d_dig.as<uint32_t>(), d_sorted.as<uint32_t>(),
                                                          d_bstart.as<uint32_t>(), d_buckets.as<g1_xyzz_t>(), s));
    TK_HIP(hipMemcpyAsync(wins_host, d_wins.p, wins_count * sizeof(g1_xyzz_t), hipMemcpyDeviceToHost, s));
    prof.finish();
    *plan_out = pl;
    return TKMK_SUCCESS;
}

// Horner over the window sums on the host: acc = 2^c * acc + W_w
static g1_xyzz_t msm_horner(const msm_plan_t &pl, const g1_xyzz_t *wins) {
    if (pl.lo_bits) {   // one bucket set reduced by rows / columns: T0 + 2^lo_bits * sum_k 2^k S_hi[k] + sum_k 2^k S_lo[k]
        g1_xyzz_t hi = G1::inf(), lo = G1::inf();
        for (int k = (int)pl.hi_bits - 1; k >= 0; k--) hi = G1::add(G1::dbl(hi), G1U::raw_to_sat(wins[1 + k]));
        for (int k = (int)pl.lo_bits - 1; k >= 0; k--) lo = G1::add(G1::dbl(lo), G1U::raw_to_sat(wins[1 + pl.hi_bits + k]));
        for (uint32_t k = 0; k < pl.lo_bits; k++) hi = G1::dbl(hi);
        return G1::add(G1::add(G1U::raw_to_sat(wins[0]), hi), lo);
    }
    g1_xyzz_t acc = G1::inf();
    for (int w = (int)pl.W - 1; w >= 0; w--) {
        for (uint32_t k = 0; k < pl.c; k++) acc = G1::dbl(acc);
        for (uint32_t part = 0; part < pl.win_parts; part++) acc = G1::add(acc, G1U::raw_to_sat(wins[w * pl.win_parts + part]));   // device records are raw (ec_u.h)
    }
    return acc;
}

// One MSM, synchronous on s.
static tkmk_error msm_one(const fr_t *scalars, const g1_affine_t *bases_mont, uint32_t n, uint32_t factor, uint32_t c_req, uint32_t bits,
                          bool scalars_mont, hipStream_t s, g1_xyzz_t *result_host) {
    tk_frame frame(s);
    std::vector<g1_xyzz_t> wins_v((size_t)MSM_MAX_WINDOWS * MSM_WIN_PARTS);
    g1_xyzz_t *wins = wins_v.data();
    msm_plan_t pl;
    TK_TRY(msm_enqueue(scalars, bases_mont, n, factor, c_req, bits, scalars_mont, s, wins, &pl, false));
    TK_HIP(hipStreamSynchronize(s));
    *result_host = msm_horner(pl, wins);
    return TKMK_SUCCESS;
}

// ---- pipelined independent MSMs -------------------------------------------------------------------
// The tail of one MSM (combine, bucket reduction: a few thousand threads of serial EC adds) is latency-bound
// and leaves most CUs idle; the prover's commits are 2^20..2^22 points, where that tail is 20-35 % of the call.
// Independent MSMs therefore run round-robin on a few internal streams (each with its own scratch arena), so
// one job's tail overlaps the next job's sort/accumulate; the host Horner of job i overlaps job i+1's kernels.
struct msm_slot {
    hipStream_t s = nullptr;
    hipEvent_t done = nullptr;
    g1_xyzz_t *wins = nullptr;  // pinned
    tk_frame *frame = nullptr;
    msm_plan_t pl;
    int job = -1;
};
struct msm_pipe_job {
    const fr_t *scalars;          // device
    const g1_affine_t *bases;     // device; converted form if !convert
    uint32_t n;
    bool convert, bases_mont;
    uint32_t factor = 1;          // precompute factor: bases hold n * factor converted points (convert must be false)
    msm_view_t sv = view_identity(), bv = view_identity();   // operand views (tkmk_msm_multi_ex)
    uint32_t c = 0;               // window width of this job (0 = the call's)
    uint32_t level_rows = 0;      // rows per level of a precomputed TABLE the base view addresses (0 = the job's own expanded points)
    bool acc_rows = false;        // `bases` is a table of accumulate-ready 128-byte rows (TKMK_BASES_ACC_READY table job; convert must be false)
};
// One pipeline set (streams, events, pinned result buffers, scratch arenas) per CALLER stream: batches issued on the same caller stream
// run one after the other (the set's lock is held from the first launch to the last result), batches issued on different caller streams
// — the resident prover's helper thread commits a round's independent polynomials on its own stream — share the device, so the
// latency-bound tails of one batch run under the additions of the other.  (r4; one process-wide set before: a second thread's batch
// waited for the whole of the first.)
struct msm_pipe_set {
    std::mutex mu;
    std::vector<msm_slot> slots;
};
static std::mutex g_pipe_sets_mu;
static std::map<hipStream_t, std::unique_ptr<msm_pipe_set>> g_pipe_sets;
static msm_pipe_set &msm_pipe_set_of(hipStream_t caller) {
    std::lock_guard<std::mutex> lk(g_pipe_sets_mu);
    std::unique_ptr<msm_pipe_set> &p = g_pipe_sets[caller];
    if (!p) p.reset(new msm_pipe_set());
    return *p;
}

// tkmk_stream_destroy (runtime.hip): the set that served a caller stream goes with it (its streams, events and pinned buffers; the scratch
// arenas of its streams stay parked like every arena until tkmk_release_scratch)
#ifdef TK_MSM_SYM_SEGMENTED
static void seg_drop_stream_flag(hipStream_t s);   // the stream's out-of-range word of asynchronous segmented calls, if it has one
#endif
void drop_pipe_set(hipStream_t caller) {
#ifdef TK_MSM_SYM_SEGMENTED
    seg_drop_stream_flag(caller);
#endif
    std::unique_ptr<msm_pipe_set> set;
    {
        std::lock_guard<std::mutex> lk(g_pipe_sets_mu);
        auto it = g_pipe_sets.find(caller);
        if (it == g_pipe_sets.end()) return;
        set = std::move(it->second);
        g_pipe_sets.erase(it);
    }
    std::lock_guard<std::mutex> lk(set->mu);   // a batch still running on the stream being destroyed finishes first
    for (msm_slot &sl : set->slots) {
        (void)hipStreamSynchronize(sl.s);
        (void)hipStreamDestroy(sl.s);
        (void)hipEventDestroy(sl.done);
        (void)hipHostFree(sl.wins);
    }
    set->slots.clear();
}

static tkmk_error msm_pipe_slots(std::vector<msm_slot> &g_slots, uint32_t want) {
    while (g_slots.size() < want) {
        msm_slot sl;
        TK_HIP(hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking));
        TK_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        TK_HIP(hipHostMalloc((void **)&sl.wins, (size_t)MSM_MAX_WINDOWS * MSM_WIN_PARTS * sizeof(g1_xyzz_t), hipHostMallocDefault));
        g_slots.push_back(sl);
    }
    return TKMK_SUCCESS;
}

static tkmk_error msm_pipe_finish(msm_slot &sl, g1_xyzz_t *results) {
    if (sl.job < 0) return TKMK_SUCCESS;
    hipError_t e = hipEventSynchronize(sl.done);
    delete sl.frame;
    sl.frame = nullptr;
    int j = sl.job;
    sl.job = -1;
    TK_HIP(e);
    results[j] = msm_horner(sl.pl, sl.wins);
    return TKMK_SUCCESS;
}

static tkmk_error msm_pipeline(const std::vector<msm_pipe_job> &jobs, uint32_t c_req, uint32_t bits, bool scalars_mont,
                               hipStream_t caller, g1_xyzz_t *results) {
    msm_pipe_set &set = msm_pipe_set_of(caller);
    std::lock_guard<std::mutex> lk(set.mu);
    const bool background = tk_stream_is_background(caller);
    std::vector<msm_slot> &g_slots = set.slots;
    const uint32_t n_streams = tk_msm_pipeline_streams();   // 3 unless TKMK_MSM_STREAMS / tkmk_msm_set_pipeline_streams say otherwise
    const uint32_t K = jobs.size() < n_streams ? (uint32_t)jobs.size() : n_streams;
    TK_TRY(msm_pipe_slots(g_slots, K));
    // work queued on the caller's stream (input uploads, shared-bases conversion) happens-before every job
    hipEvent_t ready;
    TK_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    TK_HIP(hipEventRecord(ready, caller));
    tkmk_error err = TKMK_SUCCESS;
    for (size_t j = 0; j < jobs.size() && err == TKMK_SUCCESS; j++) {
        msm_slot &sl = g_slots[j % K];
        err = msm_pipe_finish(sl, results);
        if (err != TKMK_SUCCESS) break;
        const msm_pipe_job &jb = jobs[j];
        if (j < K) {
            hipError_t e = hipStreamWaitEvent(sl.s, ready, 0);
            if (e != hipSuccess) { err = TKMK_ERR_UNKNOWN; break; }
        }
        sl.frame = new tk_frame(sl.s);
        sl.job = (int)j;
        const g1_affine_t *bm = jb.bases;
        if (jb.convert) {
            tk_scratch d_bm;
            err = d_bm.alloc((size_t)jb.n * AFF_BYTES, sl.s);
            if (err != TKMK_SUCCESS) break;
            hipLaunchKernelGGL(k_convert_bases, tk_div_up(jb.n, 256), 256, 0, sl.s, jb.bases, d_bm.as<g1_affine_t>(), (uint64_t)jb.n,
                               jb.bases_mont ? 1 : 0, jb.bv);   // the converted copy is gathered: point k at row k
            bm = d_bm.as<g1_affine_t>();
        }
        err = msm_enqueue(jb.scalars, bm, jb.n, jb.factor, jb.c ? jb.c : c_req, bits, scalars_mont, sl.s, sl.wins, &sl.pl, background, jb.sv,
                          jb.convert ? view_identity() : jb.bv, jb.convert ? 0u : jb.level_rows,
                          jb.acc_rows && !jb.convert ? (const acc_row_t *)jb.bases : nullptr);
        if (err != TKMK_SUCCESS) break;
        if (hipEventRecord(sl.done, sl.s) != hipSuccess) err = TKMK_ERR_UNKNOWN;
    }
    // drain in job order (also on error, so no frame outlives its kernels)
    {
        std::vector<msm_slot *> live;
        for (auto &sl : g_slots)
            if (sl.job >= 0) live.push_back(&sl);
        std::sort(live.begin(), live.end(), [](msm_slot *a, msm_slot *b) { return a->job < b->job; });
        for (msm_slot *sl : live) {
            if (err != TKMK_SUCCESS) (void)hipStreamSynchronize(sl->s);
            tkmk_error e2 = msm_pipe_finish(*sl, results);
            if (err == TKMK_SUCCESS) err = e2;
        }
    }
    (void)hipEventDestroy(ready);
    return err;
}

TK_API tkmk_error TK_MSM_SYM_MSM(const abi_fr *scalars, const abi_affine *bases, int msm_size, const tkmk_msm_config *cfg,
                                abi_proj *results) {
    if (!cfg || cfg->ext) return TKMK_ERR_INVALID_ARGUMENT;
    if (msm_size < 0 || cfg->batch_size < 1 || cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C ||
        cfg->precompute_factor < 0)
        return TKMK_ERR_INVALID_ARGUMENT;
    if (!results) return TKMK_ERR_INVALID_POINTER;
    TK_TRY(tk_require_device());
    const uint32_t n = (uint32_t)msm_size, batch = (uint32_t)cfg->batch_size;
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    // precompute_factor F > 1: `bases` is the table written by the _msm_precompute_bases twin with the same c / bitsize
    // (n * F converted points); it is consumed as is
    uint32_t factor = cfg->precompute_factor > 1 ? (uint32_t)cfg->precompute_factor : 1u;
    if (factor > 1) {
        if (n < 2) return TKMK_ERR_INVALID_ARGUMENT;
        // the table was made for exactly cfg->c: an MSM too small for that width (c > 16 needs the two-pass sort) cannot use it
        if (cfg->c && msm_resolve_c((uint32_t)cfg->c, n) != (uint32_t)cfg->c) return TKMK_ERR_INVALID_ARGUMENT;
        const uint32_t w_src = bits / msm_resolve_c((uint32_t)cfg->c, n) + 1;
        if (factor > w_src) factor = w_src;
    }
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    std::vector<abi_proj> host_res(batch);
    if (n == 0) {
        for (uint32_t b = 0; b < batch; b++) store_canonical(&host_res[b], G1::inf());
    } else {
        if (!scalars || !bases) return TKMK_ERR_INVALID_POINTER;
        const size_t n_bases = (cfg->are_points_shared_in_batch ? (size_t)n : (size_t)n * batch) * factor;
        tk_staged S, P;
        TK_TRY(S.in(scalars, (size_t)n * batch * FR_BYTES, cfg->are_scalars_on_device, s));
        TK_TRY(P.in(bases, n_bases * AFF_BYTES, cfg->are_points_on_device, s));
        if (n == 1) {
            // batch of one-point MSMs = batched scalar multiplication
            tk_scratch d_out;
            TK_TRY(d_out.alloc((size_t)batch * sizeof(g1_xyzz_t), s));
            hipLaunchKernelGGL(k_msm_size1, tk_div_up(batch, 128), 128, 0, s, (const fr_t *)S.dev, (const g1_affine_t *)P.dev,
                               cfg->are_points_shared_in_batch ? 1 : 0, batch, cfg->are_points_montgomery_form ? 1 : 0,
                               cfg->are_scalars_montgomery_form ? 1 : 0, d_out.as<g1_xyzz_t>());
            TK_HIP(hipGetLastError());
            std::vector<g1_xyzz_t> r(batch);
            TK_HIP(hipMemcpyAsync(r.data(), d_out.p, (size_t)batch * sizeof(g1_xyzz_t), hipMemcpyDeviceToHost, s));
            TK_HIP(hipStreamSynchronize(s));
            for (uint32_t b = 0; b < batch; b++) store_canonical(&host_res[b], r[b]);
        } else if (n <= 64 && factor == 1 && batch <= 4096) {
            // small MSMs: one launch, window sums to the host, Horner there (acc = 16 acc + W_w)
            tk_scratch d_out;
            TK_TRY(d_out.alloc((size_t)batch * SM_NW * sizeof(g1_xyzz_t), s));
            hipLaunchKernelGGL(k_msm_small, dim3(SM_NW / 4, batch), 256, 0, s, (const fr_t *)S.dev, (const g1_affine_t *)P.dev,
                               cfg->are_points_shared_in_batch ? 1 : 0, n, cfg->are_points_montgomery_form ? 1 : 0,
                               cfg->are_scalars_montgomery_form ? 1 : 0, bits, d_out.as<g1_xyzz_t>());
            TK_HIP(hipGetLastError());
            std::vector<g1_xyzz_t> r((size_t)batch * SM_NW);
            TK_HIP(hipMemcpyAsync(r.data(), d_out.p, r.size() * sizeof(g1_xyzz_t), hipMemcpyDeviceToHost, s));
            TK_HIP(hipStreamSynchronize(s));
            tk_stat_add(TK_STAT_MSM_POINTS, (uint64_t)n * batch);
            tk_stat_add(TK_STAT_MSM_CALLS, batch);
            for (uint32_t b = 0; b < batch; b++) {
                g1_xyzz_t acc = G1::inf();
                for (int w = SM_NW - 1; w >= 0; w--) {
                    for (int k = 0; k < 4; k++) acc = G1::dbl(acc);
                    acc = G1::add(acc, r[(size_t)b * SM_NW + w]);
                }
                store_canonical(&host_res[b], acc);
            }
        } else {
            tk_scratch d_bm;
            const g1_affine_t *bm = (const g1_affine_t *)P.dev;
            if (factor == 1) {
                TK_TRY(d_bm.alloc(n_bases * AFF_BYTES, s));
                tk_prof prof(s);
                hipLaunchKernelGGL(k_convert_bases, tk_div_up(n_bases, 256), 256, 0, s, (const g1_affine_t *)P.dev,
                                   d_bm.as<g1_affine_t>(), (uint64_t)n_bases, cfg->are_points_montgomery_form ? 1 : 0, view_identity());
                prof.mark("msm.convert_bases");
                prof.finish();
                TK_HIP(hipGetLastError());
                bm = d_bm.as<g1_affine_t>();
            }
            if (batch == 1) {
                g1_xyzz_t r;
                TK_TRY(msm_one((const fr_t *)S.dev, bm, n, factor, (uint32_t)cfg->c, bits, cfg->are_scalars_montgomery_form, s, &r));
                store_canonical(&host_res[0], r);
            } else {
                std::vector<msm_pipe_job> jobs(batch);
                for (uint32_t b = 0; b < batch; b++)
                    jobs[b] = {(const fr_t *)S.dev + (size_t)b * n,
                               bm + (cfg->are_points_shared_in_batch ? 0 : (size_t)b * n * factor), n, false, false, factor,
                               view_identity(), view_identity()};
                std::vector<g1_xyzz_t> r(batch);
                TK_TRY(msm_pipeline(jobs, (uint32_t)cfg->c, bits, cfg->are_scalars_montgomery_form, s, r.data()));
                for (uint32_t b = 0; b < batch; b++) store_canonical(&host_res[b], r[b]);
            }
        }
    }
    if (cfg->are_results_on_device) {
        TK_HIP(hipMemcpyAsync(results, host_res.data(), (size_t)batch * sizeof(abi_proj), hipMemcpyHostToDevice, s));
        TK_HIP(hipStreamSynchronize(s));
    } else {
        for (uint32_t b = 0; b < batch; b++) results[b] = host_res[b];
    }
    return TKMK_SUCCESS;
}

// Independent MSMs of different sizes / bases in one call (the prover's commits between two transcript
// challenges), pipelined over internal streams.  cfg's *_on_device / *_montgomery_form flags apply to every job;
// cfg->batch_size must be 1.
TK_API tkmk_error TK_MSM_SYM_MULTI(const abi_job *jobs, int n_jobs, const tkmk_msm_config *cfg, abi_proj *results) {
    if (!cfg || cfg->ext || cfg->batch_size != 1 || n_jobs < 0) return TKMK_ERR_INVALID_ARGUMENT;
    const uint32_t factor = cfg->precompute_factor > 1 ? (uint32_t)cfg->precompute_factor : 1u;   // every job: n * factor table entries
    if (cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C) return TKMK_ERR_INVALID_ARGUMENT;
    if (n_jobs == 0) return TKMK_SUCCESS;
    if (!jobs || !results) return TKMK_ERR_INVALID_POINTER;
    TK_TRY(tk_require_device());
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    std::vector<abi_proj> host_res(n_jobs);
    std::vector<msm_pipe_job> pj;
    std::vector<int> pj_index;
    std::vector<tk_staged> staged((size_t)n_jobs * 2);
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].msm_size < 0) return TKMK_ERR_INVALID_ARGUMENT;
        if (jobs[j].msm_size > 0 && (!jobs[j].scalars || !jobs[j].bases)) return TKMK_ERR_INVALID_POINTER;
    }
    for (int j = 0; j < n_jobs; j++) {
        const uint32_t n = (uint32_t)jobs[j].msm_size;
        if (n < 2) {  // empty sum / single scalar multiplication: the plain entry point handles both
            if (factor > 1 && n == 1) return TKMK_ERR_INVALID_ARGUMENT;
            tkmk_msm_config c1 = *cfg;
            c1.are_results_on_device = false;
            c1.precompute_factor = 1;
            TK_TRY(TK_MSM_SYM_MSM(jobs[j].scalars, jobs[j].bases, (int)n, &c1, &host_res[j]));
            continue;
        }
        tk_staged &S = staged[2 * j], &P = staged[2 * j + 1];
        TK_TRY(S.in(jobs[j].scalars, (size_t)n * FR_BYTES, cfg->are_scalars_on_device, s));
        uint32_t f = factor;
        if (f > 1) {
            const uint32_t w_src = bits / msm_resolve_c((uint32_t)cfg->c, n) + 1;
            if (f > w_src) f = w_src;
        }
        TK_TRY(P.in(jobs[j].bases, (size_t)n * f * AFF_BYTES, cfg->are_points_on_device, s));
        pj.push_back({(const fr_t *)S.dev, (const g1_affine_t *)P.dev, n, f == 1, cfg->are_points_montgomery_form, f, view_identity(),
                      view_identity()});
        pj_index.push_back(j);
    }
    if (!pj.empty()) {
        std::vector<g1_xyzz_t> r(pj.size());
        TK_TRY(msm_pipeline(pj, (uint32_t)cfg->c, bits, cfg->are_scalars_montgomery_form, s, r.data()));
        for (size_t k = 0; k < pj.size(); k++) store_canonical(&host_res[pj_index[k]], r[k]);
    }
    if (cfg->are_results_on_device) {
        TK_HIP(hipMemcpyAsync(results, host_res.data(), (size_t)n_jobs * sizeof(abi_proj), hipMemcpyHostToDevice, s));
        TK_HIP(hipStreamSynchronize(s));
    } else {
        for (int j = 0; j < n_jobs; j++) results[j] = host_res[j];
    }
    return TKMK_SUCCESS;
}

// Independent MSMs over VIEWS of device-resident tables (see msm_view_t): no gathered copy of the coefficient box, of the CRS
// sub-grid or of the binding-table rows is made, and with bases_form = TKMK_BASES_CONVERTED (a table that went through
// TK_MSM_SYM_CONVERT once, e.g. when the CRS was loaded) no per-call base conversion runs either.  Operands must be on the device.
#ifdef TK_MSM_SYM_MULTI_EX
static tkmk_error msm_ex_tiny(const abi_job_ex &jb, const tkmk_msm_config *cfg, int bases_form, abi_proj *out) {
    // n < 2: resolve the view on the host and hand the single term to the plain entry
    if (jb.msm_size == 0) {
        store_canonical(out, G1::inf());
        return TKMK_SUCCESS;
    }
    uint32_t bi = 0;
    if (jb.base_index) TK_HIP(hipMemcpy(&bi, jb.base_index, 4, hipMemcpyDeviceToHost));
    if (jb.base_table_len && bi >= jb.base_table_len) return TKMK_ERR_INVALID_ARGUMENT;
    fr_t sc;
    g1_affine_t pt;
    TK_HIP(hipMemcpy(&sc, jb.scalars, sizeof sc, hipMemcpyDeviceToHost));
    TK_HIP(hipMemcpy(&pt, (const g1_affine_t *)jb.bases + bi, sizeof pt, hipMemcpyDeviceToHost));
    tkmk_msm_config c1 = *cfg;
    c1.are_scalars_on_device = c1.are_points_on_device = c1.are_results_on_device = false;
    c1.precompute_factor = 1;
    c1.are_points_montgomery_form = bases_form == TKMK_BASES_MONTGOMERY;
    if (bases_form == TKMK_BASES_CONVERTED && !G1::is_inf(pt)) {   // {x R', y R'} -> plain: multiply by R'^-1 through the saturated Montgomery product
        fq_t rp;
        for (int j = 0; j < Fq::N; j++) rp.l[j] = FqP::KSATM[j];   // R' mod p, plain
        fq_t rinv = Fq::inv(Fq::to_mont(rp));                       // (R')^-1 in Montgomery form
        pt.x = Fq::mul(pt.x, rinv);                                  // plain * mont -> plain
        pt.y = Fq::mul(pt.y, rinv);
    }
    return TK_MSM_SYM_MSM((const abi_fr *)&sc, (const abi_affine *)&pt, 1, &c1, out);
}

TK_API tkmk_error TK_MSM_SYM_MULTI_EX(const abi_job_ex *jobs, int n_jobs, const tkmk_msm_config *cfg, int bases_form, abi_proj *results) {
    if (!cfg || cfg->ext || cfg->batch_size != 1 || n_jobs < 0 || cfg->precompute_factor > 1) return TKMK_ERR_INVALID_ARGUMENT;
    if (bases_form != TKMK_BASES_PLAIN && bases_form != TKMK_BASES_MONTGOMERY && bases_form != TKMK_BASES_CONVERTED && bases_form != TKMK_BASES_ACC_READY)
        return TKMK_ERR_INVALID_ARGUMENT;
    // TKMK_BASES_ACC_READY is decided per job: a table job reads 128-byte rows, every other job is taken as under TKMK_BASES_CONVERTED
    const bool acc_ready = bases_form == TKMK_BASES_ACC_READY;
    if (acc_ready) bases_form = TKMK_BASES_CONVERTED;
    if (cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C) return TKMK_ERR_INVALID_ARGUMENT;
    if (!cfg->are_scalars_on_device || !cfg->are_points_on_device) return TKMK_ERR_INVALID_ARGUMENT;   // views address resident tables
    if (n_jobs == 0) return TKMK_SUCCESS;
    if (!jobs || !results) return TKMK_ERR_INVALID_POINTER;
    TK_TRY(tk_require_device());
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    for (int j = 0; j < n_jobs; j++) {
        const abi_job_ex &jb = jobs[j];
        if (jb.msm_size < 0) return TKMK_ERR_INVALID_ARGUMENT;
        if (jb.msm_size > 0 && (!jb.scalars || !jb.bases)) return TKMK_ERR_INVALID_POINTER;
        if ((jb.scalar_cols && jb.scalar_stride < jb.scalar_cols) || (jb.base_cols && jb.base_stride < jb.base_cols)) return TKMK_ERR_INVALID_ARGUMENT;
        // the box must lie inside the table it is cut from
        if (jb.msm_size > 0 && jb.base_cols && !jb.base_index && jb.base_table_len) {
            uint64_t last = (uint64_t)((uint32_t)jb.msm_size - 1) / jb.base_cols * jb.base_stride + ((uint32_t)jb.msm_size - 1) % jb.base_cols;
            if (last >= jb.base_table_len) return TKMK_ERR_INVALID_ARGUMENT;
        }
        if (jb.base_table_len >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;   // 31-bit rows in the sort records
        if (jb.msm_size > 0 && jb.base_index && !jb.base_table_len) return TKMK_ERR_INVALID_ARGUMENT;   // an index list is never gathered unchecked
        if ((jb.table_c != 0) != (jb.table_factor != 0)) return TKMK_ERR_INVALID_ARGUMENT;
        // TKMK_BASES_ACC_READY: a job with table_c > 0 IS a table job over 128-byte rows; a one-level table (table_factor 1) would be read
        // as 96-byte records by the multi-window path, so it is refused instead
        if (acc_ready && jb.table_c != 0 && jb.table_factor < 2) return TKMK_ERR_INVALID_ARGUMENT;
        if (jb.table_factor > 1) {   // precomputed table: resident form, known level size, a window width the sort can do at this size
            if (bases_form != TKMK_BASES_CONVERTED || !jb.base_table_len || jb.table_c < 2 || jb.table_c > MSM_MAX_C) return TKMK_ERR_INVALID_ARGUMENT;
            if (jb.base_table_len * jb.table_factor >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
            if (jb.table_c > 16 && (uint64_t)jb.msm_size * jb.table_factor < (1ull << 18)) return TKMK_ERR_INVALID_ARGUMENT;
            if (acc_ready) {   // rows sit on line starts; a single term is not worth a table (the tiny path reads 96-byte records)
                if (((uintptr_t)jb.bases & (ACC_ROW_BYTES - 1)) != 0 || jb.msm_size == 1) return TKMK_ERR_INVALID_ARGUMENT;
            }
        }
    }
    tk_scratch d_flag;
    TK_TRY(d_flag.alloc(4, s));
    TK_HIP(hipMemsetAsync(d_flag.p, 0, 4, s));
    std::vector<abi_proj> host_res(n_jobs);
    std::vector<msm_pipe_job> pj;
    std::vector<int> pj_index;
    for (int j = 0; j < n_jobs; j++) {
        const abi_job_ex &jb = jobs[j];
        if (jb.msm_size < 2) {
            TK_TRY(msm_ex_tiny(jb, cfg, bases_form, &host_res[j]));
            continue;
        }
        msm_view_t sv{nullptr, jb.scalar_cols, jb.scalar_stride, 0, nullptr};
        msm_view_t bv{jb.base_index, jb.base_index ? 0u : jb.base_cols, jb.base_index ? 0u : jb.base_stride,
                      jb.base_index ? (uint32_t)jb.base_table_len : 0u, d_flag.as<uint32_t>()};
        msm_pipe_job pjob{(const fr_t *)jb.scalars, (const g1_affine_t *)jb.bases, (uint32_t)jb.msm_size, bases_form != TKMK_BASES_CONVERTED,
                          bases_form == TKMK_BASES_MONTGOMERY, 1u, sv, bv};
        if (jb.table_factor > 1) {
            pjob.factor = jb.table_factor;
            pjob.c = jb.table_c;
            pjob.level_rows = (uint32_t)jb.base_table_len;
            pjob.acc_rows = acc_ready;
        }
        pj.push_back(pjob);
        pj_index.push_back(j);
    }
    if (!pj.empty()) {
        std::vector<g1_xyzz_t> r(pj.size());
        TK_TRY(msm_pipeline(pj, (uint32_t)cfg->c, bits, cfg->are_scalars_montgomery_form, s, r.data()));
        uint32_t flag = 0;
        TK_HIP(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, s));
        TK_HIP(hipStreamSynchronize(s));
        if (flag) return TKMK_ERR_INVALID_ARGUMENT;   // a base_index entry pointed past base_table_len (the read was clamped, not faulted)
        for (size_t k = 0; k < pj.size(); k++) store_canonical(&host_res[pj_index[k]], r[k]);
    }
    if (cfg->are_results_on_device) {
        TK_HIP(hipMemcpyAsync(results, host_res.data(), (size_t)n_jobs * sizeof(abi_proj), hipMemcpyHostToDevice, s));
        TK_HIP(hipStreamSynchronize(s));
    } else {
        for (int j = 0; j < n_jobs; j++) results[j] = host_res[j];
    }
    return TKMK_SUCCESS;
}

// bases -> the library's resident form for TKMK_BASES_CONVERTED ({x R', y R'} with R' the radix of the accumulate kernel's
// unsaturated representation; (0,0) stays infinity).  In place is allowed.  One pass when a CRS is loaded replaces the
// k_convert_bases launch of every later MSM over it.
TK_API tkmk_error TK_MSM_SYM_CONVERT(const abi_affine *bases, uint64_t n, const tkmk_msm_config *cfg, abi_affine *out) {
    if (!cfg || cfg->ext) return TKMK_ERR_INVALID_ARGUMENT;
    if (n == 0) return TKMK_SUCCESS;
    if (!bases || !out) return TKMK_ERR_INVALID_POINTER;
    if (n >= (1ull << 32)) return TKMK_ERR_INVALID_ARGUMENT;
    TK_TRY(tk_require_device());
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    tk_staged P, O;
    TK_TRY(P.in(bases, (size_t)n * AFF_BYTES, cfg->are_points_on_device, s));
    TK_TRY(O.out(out, (size_t)n * AFF_BYTES, cfg->are_results_on_device, s));
    hipLaunchKernelGGL(k_convert_bases, tk_div_up(n, 256), 256, 0, s, (const g1_affine_t *)P.dev, (g1_affine_t *)O.dev, n,
                       cfg->are_points_montgomery_form ? 1 : 0, view_identity());
    TK_HIP(hipGetLastError());
    TK_TRY(O.copy_back(out, (size_t)n * AFF_BYTES, cfg->are_results_on_device, s));
    TK_HIP(hipStreamSynchronize(s));
    return TKMK_SUCCESS;
}
#endif

#ifdef TK_MSM_SYM_SEGMENTED
// calls of at most this many jobs finish on the host (see TK_MSM_SYM_SEGMENTED): below the measured crossover of the two tails
#define SEG_HOST_TAIL_MAX_JOBS 64
#define SEG_HOST_TAIL_THREADS 8   // host threads of that tail (one job is one serial chain)
// The out-of-range record of ASYNCHRONOUS segmented calls: one resident device word per caller stream that made such a call, set by the
// kernel, read and cleared by TK_MSM_SYM_SEGMENTED_STATUS.  A synchronous call keeps its flag in its own frame.  Nothing else is kept.
static std::mutex g_seg_flags_mu;
static std::map<hipStream_t, uint32_t *> g_seg_flags;
static uint32_t *seg_stream_flag(hipStream_t s, bool create) {
    std::lock_guard<std::mutex> lk(g_seg_flags_mu);
    auto it = g_seg_flags.find(s);
    if (it != g_seg_flags.end()) return it->second;
    if (!create) return nullptr;
    uint32_t *p = nullptr;
    if (hipMalloc((void **)&p, 4) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, 4) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    g_seg_flags[s] = p;
    return p;
}
static void seg_drop_stream_flag(hipStream_t s) {   // tkmk_stream_destroy, through drop_pipe_set
    std::lock_guard<std::mutex> lk(g_seg_flags_mu);
    auto it = g_seg_flags.find(s);
    if (it == g_seg_flags.end()) return;
    (void)hipFree(it->second);
    g_seg_flags.erase(it);
}

// Many ragged few-term MSMs over views / index lists of resident tables in two launches (k_msm_segmented, k_msm_segmented_finish); the
// argument rules are TK_MSM_SYM_MULTI_EX's, results[j] its bytes.  Takes the caller's stream; reads and changes no library state (the
// asynchronous form leaves its out-of-range word, see above).
TK_API tkmk_error TK_MSM_SYM_SEGMENTED(const abi_job_ex *jobs, int n_jobs, const tkmk_msm_config *cfg, int bases_form, abi_proj *results) {
    if (!cfg || cfg->ext || cfg->batch_size != 1 || n_jobs < 0 || cfg->precompute_factor > 1) return TKMK_ERR_INVALID_ARGUMENT;
    if (bases_form != TKMK_BASES_PLAIN && bases_form != TKMK_BASES_MONTGOMERY && bases_form != TKMK_BASES_CONVERTED) return TKMK_ERR_INVALID_ARGUMENT;
    if (cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C) return TKMK_ERR_INVALID_ARGUMENT;
    if (!cfg->are_scalars_on_device || !cfg->are_points_on_device) return TKMK_ERR_INVALID_ARGUMENT;   // views address resident tables
    if (n_jobs == 0) return TKMK_SUCCESS;
    if (!jobs || !results) return TKMK_ERR_INVALID_POINTER;
    TK_TRY(tk_require_device());
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    std::vector<seg_job_t> desc((size_t)n_jobs);
    uint64_t terms = 0;
    uint32_t lds_slots = 1;
    for (int j = 0; j < n_jobs; j++) {
        const abi_job_ex &jb = jobs[j];
        if (jb.msm_size < 0 || jb.msm_size > TKMK_MSM_SEGMENTED_MAX_SIZE) return TKMK_ERR_INVALID_ARGUMENT;
        if (jb.msm_size > 0 && (!jb.scalars || !jb.bases)) return TKMK_ERR_INVALID_POINTER;
        if ((jb.scalar_cols && jb.scalar_stride < jb.scalar_cols) || (jb.base_cols && jb.base_stride < jb.base_cols)) return TKMK_ERR_INVALID_ARGUMENT;
        if (jb.table_c != 0 || jb.table_factor != 0) return TKMK_ERR_INVALID_ARGUMENT;   // no table jobs here
        const uint32_t n = (uint32_t)jb.msm_size;
        // the box must lie inside the table it is cut from
        if (n > 0 && jb.base_cols && !jb.base_index && jb.base_table_len) {
            uint64_t last = (uint64_t)(n - 1) / jb.base_cols * jb.base_stride + (n - 1) % jb.base_cols;
            if (last >= jb.base_table_len) return TKMK_ERR_INVALID_ARGUMENT;
        }
        if (jb.base_table_len >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
        if (n > 0 && jb.base_index && !jb.base_table_len) return TKMK_ERR_INVALID_ARGUMENT;   // an index list is never gathered unchecked
        desc[j] = seg_job_t{(const fr_t *)jb.scalars, (const g1_affine_t *)jb.bases, jb.base_index, n, jb.scalar_cols, jb.scalar_stride,
                            jb.base_index ? 0u : jb.base_cols, jb.base_index ? 0u : jb.base_stride, jb.base_index ? (uint32_t)jb.base_table_len : 0u};
        terms += n;
        lds_slots = std::max(lds_slots, seg_slots(n));
    }
    hipStream_t s = tk_stream(cfg->stream_handle);
    const bool on_dev = cfg->are_results_on_device, async = on_dev && cfg->is_async;
    tk_frame frame(s);
    tk_scratch d_desc, d_wins, d_flag, d_res;
    TK_TRY(d_desc.alloc(desc.size() * sizeof(seg_job_t), s));
    TK_TRY(d_wins.alloc((size_t)n_jobs * SM_NW * sizeof(g1_xyzz_t), s));
    uint32_t *flag = nullptr;
    if (async) {
        flag = seg_stream_flag(s, true);
        if (!flag) return TKMK_ERR_UNKNOWN;
    } else {
        TK_TRY(d_flag.alloc(4, s));
        flag = d_flag.as<uint32_t>();
        TK_HIP(hipMemsetAsync(flag, 0, 4, s));
    }
    // The tail of a SMALL call runs on the host: one lane's chain of 4 * nw doublings, nw additions and an inversion takes 5.5 ms on this
    // device however few lanes run it (profiles/msm_segmented.json), the host's 64-bit limbs take 0.2 ms per job and thread, over a few
    // threads.  The asynchronous form has no host in its path and always takes the device tail.
    const bool host_tail = !async && n_jobs <= SEG_HOST_TAIL_MAX_JOBS;
    abi_proj *d_out = results;
    if (!on_dev && !host_tail) {
        TK_TRY(d_res.alloc((size_t)n_jobs * sizeof(abi_proj), s));
        d_out = d_res.as<abi_proj>();
    }
    // pageable source: the copy has left the host vector when this returns (as tk_staged::in relies on for every staged input)
    TK_HIP(hipMemcpyAsync(d_desc.p, desc.data(), desc.size() * sizeof(seg_job_t), hipMemcpyHostToDevice, s));
    fq_t rp;
    for (int j = 0; j < Fq::N; j++) rp.l[j] = FqP::KSATM[j];   // R' mod p of the converted form, a plain integer
    const fq_t conv = Fq::mul(Fq::inv(Fq::to_mont(rp)), Fq::r2());   // as csrc/g1check.hip: x R' * conv / R = x R
    tk_prof prof(s);
    hipLaunchKernelGGL(k_msm_segmented, dim3((uint32_t)n_jobs, SM_NW / 4), 256, lds_slots > 1 ? (size_t)4 * lds_slots * sizeof(g1k_xyzz) : 0, s,
                       d_desc.as<seg_job_t>(), bases_form, conv, cfg->are_scalars_montgomery_form ? 1 : 0, bits, lds_slots, flag, d_wins.as<g1_xyzz_t>());
    TK_HIP(hipGetLastError());
    prof.mark("msm.segmented");
    const uint32_t nw = (bits + 3) / 4;   // windows that can hold anything under cfg->bitsize
    if (!host_tail) {
        hipLaunchKernelGGL(k_msm_segmented_finish, tk_div_up((size_t)n_jobs, 64), 64, 0, s, d_wins.as<g1_xyzz_t>(), (uint32_t)n_jobs, nw, d_out);
        TK_HIP(hipGetLastError());
        prof.mark("msm.segmented_finish");
    }
    prof.finish();
    tk_stat_add(TK_STAT_MSM_SEGMENTED_JOBS, (uint64_t)n_jobs);
    tk_stat_add(TK_STAT_MSM_SEGMENTED_TERMS, terms);
    if (async) return TKMK_SUCCESS;   // the stream orders the caller's next use of `results`; out-of-range indices: TK_MSM_SYM_SEGMENTED_STATUS
    uint32_t h_flag = 0;
    TK_HIP(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, s));
    if (host_tail) {
        std::vector<g1_xyzz_t> wins((size_t)n_jobs * SM_NW);
        TK_HIP(hipMemcpyAsync(wins.data(), d_wins.p, wins.size() * sizeof(g1_xyzz_t), hipMemcpyDeviceToHost, s));
        TK_HIP(hipStreamSynchronize(s));
        if (h_flag) return TKMK_ERR_INVALID_ARGUMENT;
        std::vector<abi_proj> host_res((size_t)n_jobs);
        auto tail = [&](int first, int step) {   // jobs first, first + step, ...: independent chains of ~0.2 ms each
            for (int j = first; j < n_jobs; j += step) {
                g1_xyzz_t acc = G1::inf();
                for (int w = (int)nw - 1; w >= 0; w--) {
                    for (int k = 0; k < 4; k++) acc = G1::dbl(acc);
                    acc = G1::add(acc, wins[(size_t)j * SM_NW + w]);
                }
                store_canonical(&host_res[j], acc);
            }
        };
        const int workers = std::min(n_jobs, SEG_HOST_TAIL_THREADS);
        std::vector<std::thread> pool;
        for (int t = 1; t < workers; t++) pool.emplace_back(tail, t, workers);
        tail(0, workers);
        for (std::thread &t : pool) t.join();
        if (on_dev) {
            TK_HIP(hipMemcpyAsync(results, host_res.data(), host_res.size() * sizeof(abi_proj), hipMemcpyHostToDevice, s));
            TK_HIP(hipStreamSynchronize(s));
        } else {
            for (int j = 0; j < n_jobs; j++) results[j] = host_res[j];
        }
        return TKMK_SUCCESS;
    }
    if (!on_dev) TK_HIP(hipMemcpyAsync(results, d_out, (size_t)n_jobs * sizeof(abi_proj), hipMemcpyDeviceToHost, s));
    TK_HIP(hipStreamSynchronize(s));
    return h_flag ? TKMK_ERR_INVALID_ARGUMENT : TKMK_SUCCESS;   // a base_index entry pointed past base_table_len (the read was clamped, not faulted)
}
TK_API tkmk_error TK_MSM_SYM_SEGMENTED_STATUS(tkmk_stream stream) {
    hipStream_t s = tk_stream(stream);
    uint32_t *flag = seg_stream_flag(s, false);
    if (!flag) return TKMK_SUCCESS;   // no asynchronous segmented call was made on this stream
    uint32_t h_flag = 0;
    TK_HIP(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, s));
    if (hipStreamSynchronize(s) != hipSuccess) return TKMK_ERR_UNKNOWN;
    if (!h_flag) return TKMK_SUCCESS;
    TK_HIP(hipMemsetAsync(flag, 0, 4, s));
    TK_HIP(hipStreamSynchronize(s));
    return TKMK_ERR_INVALID_ARGUMENT;
}
#endif

// Expanded base table for precompute_factor F = cfg->precompute_factor (ICICLE's msm_precompute_bases): out holds
// n * F' points, F' = min(F, windows), out[j * n + i] = 2^(c W' j) P_i with W' = ceil(windows / F') windows per group, in
// the library's converted form (only meaningful as the `bases` of a later MSM with the same c, bitsize and factor).
// The MSM over the table is the ordinary pipeline on n * F' points and W' windows (k_digits routes window j W' + t of
// scalar i to window t of point (j, i)); same bucket additions, no base conversion, fewer buckets.
TK_API tkmk_error TK_MSM_SYM_PRECOMPUTE(const abi_affine *bases, int n_points, const tkmk_msm_config *cfg, abi_affine *output_bases) {
    if (!cfg || cfg->ext || n_points < 2 || cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C ||
        cfg->precompute_factor < 1)
        return TKMK_ERR_INVALID_ARGUMENT;
    if (!bases || !output_bases) return TKMK_ERR_INVALID_POINTER;
    TK_TRY(tk_require_device());
    const uint32_t n = (uint32_t)n_points;
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    // an explicit window width is taken as given (a table for tkmk_msm_multi_ex's table jobs is made for ONE c, whatever the
    // table's size); 0 = the width bls12_381_msm would choose for an MSM of n_points
    const uint32_t c = cfg->c ? (uint32_t)cfg->c : msm_resolve_c(0, n);
    const uint32_t w_src = bits / c + 1;
    uint32_t factor = (uint32_t)cfg->precompute_factor;
    if (factor > w_src) factor = w_src;
    if ((uint64_t)n * factor >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
    const uint32_t wg = (w_src + factor - 1) / factor;
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    tk_staged P, O;
    TK_TRY(P.in(bases, (size_t)n * AFF_BYTES, cfg->are_points_on_device, s));
    TK_TRY(O.out(output_bases, (size_t)n * factor * AFF_BYTES, cfg->are_results_on_device, s));
    hipLaunchKernelGGL(k_precompute_bases, tk_div_up(n, 128), 128, 0, s, (const g1_affine_t *)P.dev, (g1_affine_t *)O.dev, (uint64_t)n,
                       cfg->are_points_montgomery_form ? 1 : 0, factor, c * wg);
    TK_HIP(hipGetLastError());
    TK_TRY(O.copy_back(output_bases, (size_t)n * factor * AFF_BYTES, cfg->are_results_on_device, s));
    TK_HIP(hipStreamSynchronize(s));
    return TKMK_SUCCESS;
}

#ifdef TK_MSM_SYM_PRECOMPUTE_ACC
// The same table as accumulate-ready rows (TKMK_BASES_ACC_READY): n * F' records of 128 bytes, row r of the table at out + 128 r, written
// on the device (`out` is device memory on a 128-byte boundary).  out == NULL: only *out_bytes is set.
TK_API tkmk_error TK_MSM_SYM_PRECOMPUTE_ACC(const abi_affine *bases, uint64_t n_points, const tkmk_msm_config *cfg, void *out, uint64_t *out_bytes) {
    if (!cfg || cfg->ext || n_points < 2 || n_points >= (1ull << 31) || cfg->bitsize < 0 || cfg->bitsize > 255 || cfg->c < 0 || cfg->c > MSM_MAX_C ||
        cfg->precompute_factor < 1)
        return TKMK_ERR_INVALID_ARGUMENT;
    const uint32_t n = (uint32_t)n_points;
    const uint32_t bits = cfg->bitsize ? (uint32_t)cfg->bitsize : (uint32_t)TK_MSM_SCALAR_BITS;
    const uint32_t c = cfg->c ? (uint32_t)cfg->c : msm_resolve_c(0, n);
    const uint32_t w_src = bits / c + 1;
    uint32_t factor = (uint32_t)cfg->precompute_factor;
    if (factor > w_src) factor = w_src;
    if ((uint64_t)n * factor >= (1ull << 31)) return TKMK_ERR_INVALID_ARGUMENT;
    if (out_bytes) *out_bytes = (uint64_t)n * factor * ACC_ROW_BYTES;
    if (!out) return out_bytes ? TKMK_SUCCESS : TKMK_ERR_INVALID_POINTER;
    if (!bases) return TKMK_ERR_INVALID_POINTER;
    if (((uintptr_t)out & (ACC_ROW_BYTES - 1)) != 0) return TKMK_ERR_INVALID_ARGUMENT;
    TK_TRY(tk_require_device());
    const uint32_t wg = (w_src + factor - 1) / factor;
    hipStream_t s = tk_stream(cfg->stream_handle);
    tk_frame frame(s);
    tk_staged P;
    TK_TRY(P.in(bases, (size_t)n * AFF_BYTES, cfg->are_points_on_device, s));
    hipLaunchKernelGGL(k_precompute_bases_acc, tk_div_up(n, 128), 128, 0, s, (const g1_affine_t *)P.dev, (acc_row_t *)out, (uint64_t)n,
                       cfg->are_points_montgomery_form ? 1 : 0, factor, c * wg);
    TK_HIP(hipGetLastError());
    TK_HIP(hipStreamSynchronize(s));
    return TKMK_SUCCESS;
}
#endif

}  // namespace TK_MSM_NS
