// tkmk_crs_locate.hpp — the search behind the locate pass of the CRS audit (host/tkmk_crs_audit.hpp, crs-check --locate): which record makes
// a failed check fail?  Pure host code: no device, no pairing, no field arithmetic — an extent, a predicate, a count of its calls.
// Every equation of the audit is a sum over records with fixed weights, so a failing check splits into two half-checks over the SAME
// weights whose sums add up to the failing one: when the lower half passes, the upper half fails and need not be evaluated.  One predicate
// call per level therefore finds the FIRST bad index, in ceil(log2 n) calls, none of them over the whole extent (that one has failed
// already: it is why the search runs).
//   first_bad       [0, n), fails(lo, hi) = "the check restricted to [lo, hi) fails"
//   first_bad_cell  rows x cols, fails(r0, r1, c0, c1): rows first over all columns, then the columns of the row found
//   meet            the record that the first failing relation along Y and the first failing relation along X of xy_powers have in common
// Under a predicate that is not additive (the callers' are, except with probability ~ 1 / r) the result is still an index of the extent.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tkmk {
namespace crs_locate {

inline size_t ceil_log2(size_t n) {
    size_t k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

// the first index of [0, n) whose terms make the check fail, GIVEN that it fails over [0, n); n >= 1.  calls += the predicate calls made
// (at most ceil_log2(n)).
template <class Fails>
inline size_t first_bad(size_t n, Fails &&fails, size_t &calls) {
    size_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;   // the lower part is the smaller one: both are at most ceil(size / 2)
        calls++;
        if (fails(lo, mid))
            hi = mid;
        else
            lo = mid;
    }
    return lo;
}

struct Cell {
    size_t row, col;
};
// the first failing row (over all columns), then the first failing column of that row: at most ceil_log2(rows) + ceil_log2(cols) calls
template <class Fails>
inline Cell first_bad_cell(size_t rows, size_t cols, Fails &&fails, size_t &calls) {
    const size_t r = first_bad(rows, [&](size_t lo, size_t hi) { return fails(lo, hi, (size_t)0, cols); }, calls);
    const size_t c = first_bad(cols, [&](size_t lo, size_t hi) { return fails(r, r + 1, lo, hi); }, calls);
    return Cell{r, c};
}

// xy_powers, rs_y records per row.  A relation is named by its source record: along Y it ties (a, b) to (a, b + 1), along X (a, b) to
// (a + 1, b); one that fails has a wrong source or a wrong target.  The record both first failing relations touch, or SIZE_MAX when they
// touch none in common (then no single record explains both).
inline size_t meet(size_t y_source, size_t x_source, size_t rs_y) {
    const size_t y[2] = {y_source, y_source + 1}, x[2] = {x_source, x_source + rs_y};
    for (size_t u : y)
        for (size_t v : x)
            if (u == v) return u;
    return SIZE_MAX;
}

}  // namespace crs_locate
}  // namespace tkmk
