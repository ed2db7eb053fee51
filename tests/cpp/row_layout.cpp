// row_layout.hpp against a brute-force count.  For totals drawn from {0, 1, 63, 64, 65, 128} over 0 .. ADMM_MAX_SHAPES + 1 rows: row_blocks
// is the number of 64-item blocks counted one by one, blocks_before the count over the rows before; every block index below the sum of
// the rows' blocks maps to exactly one row -- the one whose range holds it -- with that row's items and blocks before it, the first
// index at the sum and one far beyond map to none, and the bound on the partial blocks holds.  Stand-alone: includes row_layout.hpp and
// admm_kinds.h alone, exits 0 when every case agrees.
#include "row_layout.hpp"
#include "admm_kinds.h"

#include <cstdio>
#include <vector>

using namespace admm_layout;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the blocks a row of `total` items needs, one item at a time
static long long brute_blocks(long long total) {
    long long nb = 0;
    for (long long i = 0; i < total; ++i) if (i % 64 == 0) ++nb;
    return nb;
}

static void check(const std::vector<long long> &total) {
    const int rows = (int)total.size();
    std::vector<long long> first(rows + 1, 0), items(rows + 1, 0);      // by brute force: the first block and the first item of every row
    for (int q = 0; q < rows; ++q) { first[q + 1] = first[q] + brute_blocks(total[q]); items[q + 1] = items[q] + total[q]; }
    for (int q = 0; q < rows; ++q) CHECK(row_blocks(total[q]) == brute_blocks(total[q]));
    for (int q = 0; q <= rows; ++q) CHECK(blocks_before(total.data(), q) == first[q]);
    CHECK(first[rows] <= partial_blocks_bound(items[rows], rows));
    for (long long B = 0; B < first[rows]; ++B) {
        int holders = 0, holder = -1;
        for (int q = 0; q < rows; ++q) if (first[q] <= B && B < first[q + 1]) { ++holders; holder = q; }
        long long base = -1, blk0 = -1;
        const int row = block_row(total.data(), rows, B, base, blk0);
        CHECK(holders == 1 && row == holder);
        if (row >= 0) { CHECK(base == items[row] && blk0 == first[row]); CHECK((B - blk0) * 64 < total[row]); }
    }
    for (long long B : {first[rows], first[rows] + 1, first[rows] + 1000000}) {
        long long base = -1, blk0 = -1;
        CHECK(block_row(total.data(), rows, B, base, blk0) == -1);
        CHECK(base == items[rows] && blk0 == first[rows]);
    }
}

int main() {
    const long long draw[6] = {0, 1, 63, 64, 65, 128};
    CHECK(ROW_BLOCK == 64);
    check({});
    // every pair and triple of the six totals, every single one
    for (long long a : draw) { check({a}); for (long long b : draw) { check({a, b}); for (long long c : draw) check({a, b, c}); } }
    // longer lists up to the largest the library has, ADMM_MAX_SHAPES + 1 rows: a fixed linear congruential draw, and all rows alike
    unsigned s = 12345u;
    for (int rows = 4; rows <= ADMM_MAX_SHAPES + 1; ++rows) {
        std::vector<long long> t(rows);
        for (long long &v : t) { s = s * 1664525u + 1013904223u; v = draw[(s >> 16) % 6]; }
        check(t);
    }
    for (long long a : draw) check(std::vector<long long>(ADMM_MAX_SHAPES + 1, a));
    if (failures) { std::printf("row_layout: %d checks failed\n", failures); return 1; }
    std::printf("row_layout: ok\n");
    return 0;
}
