// r1cs_library.h — the device-resident constraint library behind tkmk_r1cs_library_* (witness.hip builds, evaluates and frees it;
// crsaudit.hip reads it): CSR of A / B / C of every subcircuit kind, coefficients kept in Montgomery form.
#pragma once
#include <vector>

#include "common.h"

struct tkmk_r1cs_library {
    uint32_t n_sub = 0, max_rows = 0;
    uint32_t *d_rowptr = nullptr;    // concatenated row_ptr arrays, (n_rows + 1) each, order [sub][matrix]
    uint32_t *d_wire = nullptr;      // concatenated wire arrays
    fr_t *d_coeff = nullptr;         // concatenated coefficients, Montgomery form
    uint32_t *d_desc = nullptr;      // per (sub, matrix): {rowptr base, entry base}; per sub: n_rows, n_wires  -> 8 u32 per sub
    std::vector<uint32_t> n_rows, n_wires;
};
