// g1check.hip — batched membership test of G1 records behind tkmk_g1_check (include/tkmk.h): is every record of a table of the reference
// string the all-zero record (infinity) or a canonically stored point of the prime-order subgroup of E(Fq): y^2 = x^3 + 4?
// No reference counterpart: the reference takes its CRS as downloaded (prove/src/sigma_source.rs) and checks the power structure inside the
// ceremony only (setup/mpc-setup/src/utils.rs:1447-1476).
//
// Per record, in this order, the first failure being the verdict (later tests mean nothing after it):
//   infinity      all 24 words zero: counted, passes
//   canonical     the stored integer of x or of y is >= p (in every form: x + p is NOT accepted as x)
//   curve         y^2 = x^3 + 4 in Montgomery arithmetic (the conversions of k_g1ntt_load)
//   subgroup      [r]P = infinity, decided by the endomorphism test of M. Scott (ePrint 2021/1130, section 4): with phi(x, y) = (beta x, y) and
//                 z the curve parameter, P on the curve is in the subgroup iff phi(P) = -[z^2]P.  |z| = 0xd201000000010000 has 6 set bits:
//                 two successive [|z|] chains, 126 doublings + 10 additions against the 255 + 133 of the chain over r, then a cross-multiplied
//                 comparison in XYZZ (no inversion).  The chain runs on points of SMALL order (the cofactor is 3 * 11^2 * 10177^2 * 859267^2 *
//                 52437899^2) and meets acc = P, acc = -P and acc = infinity on the way: it uses the complete formulas of ec.h.
// beta is the cube root of unity in Fq whose eigenvalue on the subgroup is -z^2 mod r (the other root accepts nothing).  It is DERIVED on the
// host at first use — c^((p - 1) / 3) for the first c that is no cube, then whichever of {beta, beta^2} satisfies the rule on the generator —
// not typed in; tests/test_g1_torsion.py derives it again with big integers and compares the rule with [r]P on every kind of input.
//
// One lane per record; the scalar is the same in every lane, so a wave does not diverge inside the chain, and a wave whose lanes are all
// infinity / already failed skips it.  Counters: one ballot per verdict and wave, lane 0 adds the population counts that are not zero (a clean
// table issues no atomic at all); first_bad is a 64-bit atomic min of the wave's lowest failing index.
#include <mutex>

#include "common.h"

namespace {

constexpr uint64_t BLS_Z_ABS = 0xd201000000010000ull;   // |z|; z itself is negative, z^2 = |z|^2

struct g1check_counters {   // device cell, one per call
    unsigned long long n_infinity, n_noncanonical, n_off_curve, n_not_in_subgroup, first_bad;
};

__device__ __forceinline__ bool fq_at_least_p(const fq_t &a) {
    fq_t t;
    return Fq::sub_raw(t, a, Fq::modulus()) == 0;
}

// [|z|]([|z|] P) for P != infinity (host and device: the host runs it once, on the generator, to choose beta)
FF_HD g1_xyzz_t g1_mul_z_squared(const g1_affine_t &p, uint64_t z_abs) {
    g1_xyzz_t q = G1::from_affine(p);
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        g1_xyzz_t acc = q;
#pragma unroll 1
        for (int bit = 62; bit >= 0; bit--) {   // bit 63 of |z| is set: acc starts at q
            acc = G1::dbl(acc);
            if ((z_abs >> bit) & 1) acc = G1::add(acc, q);
        }
        q = acc;
    }
    return q;
}
// (beta x, y) == -q, cross-multiplied: beta x ZZ = X and y ZZZ = -Y; q = infinity never equals the finite phi(P)
FF_HD bool g1_phi_equals_neg(const g1_affine_t &p, const fq_t &beta, const g1_xyzz_t &q) {
    if (G1::is_inf(q)) return false;
    const bool ex = Fq::eq(Fq::mul(Fq::mul(beta, p.x), q.zz), q.x);
    const bool ey = Fq::is_zero(Fq::add(Fq::mul(p.y, q.zzz), q.y));
    return ex && ey;
}

__global__ __launch_bounds__(128) void k_g1_check(const g1_affine_t *__restrict__ in, uint64_t n, uint32_t cols, uint32_t stride, int form, fq_t conv,
                                                 fq_t beta, uint64_t z_abs, uint8_t *__restrict__ verdict, g1check_counters *__restrict__ ctr) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e < n;
    int v = 0;
    bool inf = false, chain = false;
    g1_affine_t p;
    p.x = Fq::zero(), p.y = Fq::zero();
    if (live) {
        uint64_t at = e;
        if (cols) {
            const uint64_t a = e / cols;
            at = a * stride + (e - a * cols);
        }
        p = tk_load(in + at);
        inf = G1::is_inf(p);
        if (!inf) {
            if (fq_at_least_p(p.x) || fq_at_least_p(p.y)) {
                v = TKMK_G1_BAD_NONCANONICAL;
            } else {
                if (form == TKMK_BASES_PLAIN) p.x = Fq::to_mont(p.x), p.y = Fq::to_mont(p.y);
                else if (form == TKMK_BASES_CONVERTED) p.x = Fq::mul(p.x, conv), p.y = Fq::mul(p.y, conv);   // x R' * (R^2 / R') / R = x R
                const fq_t two = Fq::dbl(Fq::one());
                const fq_t rhs = Fq::add(Fq::mul(Fq::sqr(p.x), p.x), Fq::dbl(two));
                if (!Fq::eq(Fq::sqr(p.y), rhs)) v = TKMK_G1_BAD_OFF_CURVE;
                else chain = true;
            }
        }
    }
    if (chain) {
        const g1_xyzz_t q = g1_mul_z_squared(p, z_abs);
        if (!g1_phi_equals_neg(p, beta, q)) v = TKMK_G1_BAD_NOT_IN_SUBGROUP;
    }
    if (live && verdict) verdict[e] = (uint8_t)v;
    // per-wave reduction: the lanes of a wave hold consecutive indices, so the lowest failing lane is the wave's lowest failing index
    const unsigned long long b_inf = __ballot(inf), b_nc = __ballot(v == TKMK_G1_BAD_NONCANONICAL), b_oc = __ballot(v == TKMK_G1_BAD_OFF_CURVE),
                             b_ns = __ballot(v == TKMK_G1_BAD_NOT_IN_SUBGROUP);
    const unsigned lane = threadIdx.x & (warpSize - 1);
    if (lane == 0) {
        if (b_inf) atomicAdd(&ctr->n_infinity, (unsigned long long)__popcll(b_inf));
        if (b_nc) atomicAdd(&ctr->n_noncanonical, (unsigned long long)__popcll(b_nc));
        if (b_oc) atomicAdd(&ctr->n_off_curve, (unsigned long long)__popcll(b_oc));
        if (b_ns) atomicAdd(&ctr->n_not_in_subgroup, (unsigned long long)__popcll(b_ns));
        const unsigned long long bad = b_nc | b_oc | b_ns;
        if (bad) atomicMin(&ctr->first_bad, (unsigned long long)(e + (uint64_t)(__ffsll((long long)bad) - 1)));
    }
}

// a / 3 for the N-limb integer a (exact for p - 1: p = 1 mod 3)
void limbs_div3(uint32_t *a, int nl) {
    uint64_t rem = 0;
    for (int i = nl - 1; i >= 0; i--) {
        const uint64_t cur = (rem << 32) | a[i];
        a[i] = (uint32_t)(cur / 3);
        rem = cur % 3;
    }
}

// beta in Montgomery form; false if the derivation does not close on the generator (never, for this curve: a build that breaks the host
// arithmetic must not turn into a kernel that accepts nothing or everything)
bool derive_beta(fq_t &beta_out) {
    static const uint32_t GX[12] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu,
                                    0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u};   // setup/mpc-setup/src/conversions.rs:68-79
    static const uint32_t GY[12] = {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu,
                                    0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u};
    uint32_t ex[Fq::N];
    for (int i = 0; i < Fq::N; i++) ex[i] = bls12_381_fq_params::MOD[i];
    ex[0] -= 1;   // p is odd
    limbs_div3(ex, Fq::N);
    fq_t w = Fq::one();
    for (uint32_t c = 2; c < 16 && Fq::eq(w, Fq::one()); c++) {   // c^((p - 1) / 3), most significant bit first
        const fq_t base = Fq::from_u32(c);
        w = Fq::one();
        for (int bit = 32 * Fq::N - 1; bit >= 0; bit--) {
            w = Fq::sqr(w);
            if ((ex[bit >> 5] >> (bit & 31)) & 1u) w = Fq::mul(w, base);
        }
    }
    if (Fq::eq(w, Fq::one())) return false;
    g1_affine_t g;
    for (int i = 0; i < Fq::N; i++) g.x.l[i] = GX[i], g.y.l[i] = GY[i];
    g.x = Fq::to_mont(g.x), g.y = Fq::to_mont(g.y);
    const g1_xyzz_t q = g1_mul_z_squared(g, BLS_Z_ABS);
    const fq_t w2 = Fq::sqr(w);
    const bool a = g1_phi_equals_neg(g, w, q), b = g1_phi_equals_neg(g, w2, q);
    if (a == b) return false;
    beta_out = a ? w : w2;
    return true;
}

}  // namespace

TK_API tkmk_error tkmk_g1_check(const tkmk_g1_affine *points_dev, int bases_form, uint64_t n, uint32_t cols, uint32_t stride, uint8_t *verdict_dev,
                                tkmk_g1_check_report *report_host, tkmk_stream stream) {
    if (!report_host || (!points_dev && n)) return TKMK_ERR_INVALID_POINTER;
    if (bases_form != TKMK_BASES_PLAIN && bases_form != TKMK_BASES_MONTGOMERY && bases_form != TKMK_BASES_CONVERTED) return TKMK_ERR_INVALID_ARGUMENT;
    if ((cols == 0) != (stride == 0) || stride < cols) return TKMK_ERR_INVALID_ARGUMENT;
    if (n >= (1ull << 38)) return TKMK_ERR_INVALID_ARGUMENT;   // the grid of 128-lane workgroups stays below 2^31
    tkmk_g1_check_report rep{};
    rep.first_bad = UINT64_MAX;
    if (n == 0) {
        *report_host = rep;
        return TKMK_SUCCESS;
    }
    TK_TRY(tk_require_device());
    static fq_t beta;
    static bool beta_ok = false;
    static std::once_flag beta_once;
    std::call_once(beta_once, [] { beta_ok = derive_beta(beta); });
    if (!beta_ok) return TKMK_ERR_UNKNOWN;
    hipStream_t s = tk_stream(stream);
    tk_frame frame(s);
    tk_scratch d_ctr;
    TK_TRY(d_ctr.alloc(sizeof(g1check_counters), s));
    g1check_counters *ctr = d_ctr.as<g1check_counters>();
    TK_HIP(hipMemsetAsync(ctr, 0, offsetof(g1check_counters, first_bad), s));
    TK_HIP(hipMemsetAsync(&ctr->first_bad, 0xff, sizeof(ctr->first_bad), s));
    fq_t rp;
    for (int j = 0; j < Fq::N; j++) rp.l[j] = bls12_381_fq_params::KSATM[j];   // R' mod p of the converted form, a plain integer
    const fq_t conv = Fq::mul(Fq::inv(Fq::to_mont(rp)), Fq::r2());
    tk_prof prof(s);
    hipLaunchKernelGGL(k_g1_check, tk_div_up(n, 128), 128, 0, s, (const g1_affine_t *)points_dev, n, cols, stride, bases_form, conv, beta, BLS_Z_ABS,
                       verdict_dev, ctr);
    TK_HIP(hipGetLastError());
    prof.mark("g1.check");
    prof.finish();
    g1check_counters h;
    TK_HIP(hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, s));
    TK_HIP(hipStreamSynchronize(s));   // the report is on the host when the call returns
    rep.n_checked = n;
    rep.n_infinity = h.n_infinity, rep.n_noncanonical = h.n_noncanonical, rep.n_off_curve = h.n_off_curve;
    rep.n_not_in_subgroup = h.n_not_in_subgroup, rep.first_bad = h.first_bad;
    *report_host = rep;
    return TKMK_SUCCESS;
}
