// hostcheck_ffu_raw.cpp — TEST-ONLY: ffu::mul / mul_add / mul_add<true> / sqr (csrc/ffu.h) on RAW limb operands, compiled for the host with
// every FFU_ASSERT live; the host twin of tkmk_diag_ffu (csrc/diag.hip).  Built on its own by build_ffu_raw.py.
#include <stddef.h>

#include "ffu.h"

template <class FU>
static void run(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n) {
    const int L = FU::L;
    for (size_t i = 0; i < n; i++) {
        typename FU::E x[4], r;
        const uint32_t *src[4] = {a, b, c, d};
        for (int k = 0; k < 4; k++)
            for (int l = 0; l < L; l++) x[k].l[l] = src[k] ? src[k][L * i + l] : 0u;
        if (op == 0) r = FU::mul(x[0], x[1]);
        else if (op == 1) r = FU::template mul_add<false>(x[0], x[1], x[2], x[3]);
        else if (op == 2) r = FU::template mul_add<true>(x[0], x[1], x[2], x[3]);
        else r = FU::sqr(x[0]);
        for (int l = 0; l < L; l++) out[L * i + l] = r.l[l];
    }
}

extern "C" {
// curve 0 = BLS12-381 Fq (14 x 29), 1 = BN254 Fq (10 x 28); op as tkmk_diag_ffu; operands an op does not read may be NULL
int hc_ffu_raw(int curve, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n) {
    if (curve < 0 || curve > 1 || op < 0 || op > 3) return 1;
    if (curve == 0) run<ffu<bls12_381_fq_params>>(op, a, b, c, d, out, n);
    else run<ffu<bn254_fq_params>>(op, a, b, c, d, out, n);
    return 0;
}
}
