// test driver for host/tkmk_crs_locate.hpp (CPU only: the header has no device, pairing or field dependency, and neither has this file)
//   crs_locate_driver < CASES
// CASES, whitespace-separated, any number of
//   1 n k i_1 .. i_k               first_bad over [0, n) with the fake predicate "a range fails iff it meets {i_1 .. i_k}"
//   2 rows cols k r_1 c_1 .. r_k c_k   first_bad_cell over rows x cols, a box fails iff it holds one of the cells
//   3 y_source x_source rs_y       meet
// prints per case one line:  `index calls`,  `row col calls`,  `index` (-1: the relations do not meet).  A predicate call over an empty
// range, past the extent, or over the whole extent is a bug of the search: exit code 1 with a message.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "tkmk_crs_locate.hpp"

using namespace tkmk::crs_locate;

template <class T>
static T next() {
    T v;
    if (!(std::cin >> v)) throw std::runtime_error("the cases end early");
    return v;
}

int main() {
    try {
        int kind;
        while (std::cin >> kind) {
            if (kind == 1) {
                const size_t n = next<size_t>();
                std::vector<size_t> bad(next<size_t>());
                for (size_t &b : bad) b = next<size_t>();
                if (n == 0) throw std::runtime_error("an extent is at least 1");
                size_t calls = 0;
                const size_t at = first_bad(n, [&](size_t lo, size_t hi) {
                    if (lo >= hi || hi > n || hi - lo == n) throw std::runtime_error("first_bad asked for a range it must not ask for");
                    for (size_t b : bad)
                        if (b >= lo && b < hi) return true;
                    return false;
                }, calls);
                printf("%zu %zu\n", at, calls);
            } else if (kind == 2) {
                const size_t rows = next<size_t>(), cols = next<size_t>();
                std::vector<Cell> bad(next<size_t>());
                for (Cell &b : bad) b.row = next<size_t>(), b.col = next<size_t>();
                if (rows == 0 || cols == 0) throw std::runtime_error("an extent is at least 1");
                size_t calls = 0;
                const Cell at = first_bad_cell(rows, cols, [&](size_t r0, size_t r1, size_t c0, size_t c1) {
                    if (r0 >= r1 || r1 > rows || c0 >= c1 || c1 > cols || (r1 - r0 == rows && c1 - c0 == cols))
                        throw std::runtime_error("first_bad_cell asked for a box it must not ask for");
                    for (const Cell &b : bad)
                        if (b.row >= r0 && b.row < r1 && b.col >= c0 && b.col < c1) return true;
                    return false;
                }, calls);
                printf("%zu %zu %zu\n", at.row, at.col, calls);
            } else if (kind == 3) {
                const size_t y = next<size_t>(), x = next<size_t>(), rs_y = next<size_t>();
                const size_t at = meet(y, x, rs_y);
                printf("%lld\n", at == SIZE_MAX ? -1ll : (long long)at);
            } else {
                throw std::runtime_error("unknown case kind");
            }
        }
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "crs_locate_driver: %s\n", e.what());
        return 1;
    }
}
