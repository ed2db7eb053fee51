// row_layout.hpp -- where the 64-item blocks of several rows sit when every row is cut into blocks of its own and the rows' blocks follow
// each other: row q's blocks start at the sum over q' < q of ceil(total[q'] / 64), its last block is padded.  The one statement of that
// rule, shared by the device (kernels_reaction.hpp: the per-entry and per-body partial sums; kernels_attach.hpp) and the host
// (abi_reaction.inc, abi_attach.inc: the sizes of the partial buffers and grids).  Integers only.  Extension, no reference counterpart.
#pragma once

#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_layout {

constexpr int ROW_BLOCK = 64;

ADMM_HD long long row_blocks(const long long total) { return (total + ROW_BLOCK - 1) / ROW_BLOCK; }

// the row of block B among the first n_rows rows, -1: B lies at or beyond their last block; -> base, blk0: the items and the blocks of the
// rows before that row (of all n_rows rows when there is none)
ADMM_HD int block_row(const long long *total, const int n_rows, const long long B, long long &base, long long &blk0) {
    base = 0; blk0 = 0;
    for (int q = 0; q < n_rows; ++q) {
        const long long nb = row_blocks(total[q]);
        if (B < blk0 + nb) return q;
        blk0 += nb; base += total[q];
    }
    return -1;
}

// the blocks of the rows before `row`: block_row's walk with a block no row reaches
ADMM_HD long long blocks_before(const long long *total, const int row) {
    long long base, blk0;
    block_row(total, row, 0x7fffffffffffffffll, base, blk0);
    return blk0;
}

// a bound on the blocks of `rows` rows that hold at most `items` items between them: every row pads at most one block
ADMM_HD long long partial_blocks_bound(const long long items, const int rows) { return row_blocks(items) + rows; }

} // namespace admm_layout
