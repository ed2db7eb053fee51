// kernels_attach.hpp -- rigid attachments (attach.hpp): the device side.  Extension, no reference counterpart; no product path launches
// any of this unless an ANCHOR batch is attached to a rigid body (admm_hip_attach_anchors).  No atomics, fixed orders: two runs give the
// same bits.  All on the context's stream, eager, outside the captured graphs (abi_rigid.inc's two hooks).
//
// The tables (uploaded by the host whenever the set of attachments changes, abi_attach.inc):
//   bat  [n_slots]  AttachBatchDev, one per attached batch in ascending batch index: the batch's own device arrays (idx, w2, active, u,
//                   z, targets), its local offsets [n][3], its element count n and its body
//   blk  [n_tblk]   AttachBlock { slot, first }: 64 consecutive elements of one attached batch, for the targets
//   el_slot, el_elem [sum of n]   the attached elements sorted by (body, batch index, element), for the load; total [ADMM_MAX_SHAPES]
//                   the number of them per body (0: none), carry [ADMM_MAX_SHAPES] whether the body carries a batch at all
//
// At the very start of a step, behind rigid_pose_kernel:
//   attach_targets_kernel   one lane per attached element of all attached batches, block -> (batch, first element) through blk:
//                           t = c + R r from rec[body] (one uniform read per block) and the element's offset; three doubles into the
//                           batch's targets [n][3] (lane i at 24 i bytes: the wave's stores cover 1.5 KiB without a gap), nothing else
// Behind the frame's epilogue, before rigid_integrate_kernel:
//   attach_partial_kernel   one wave per 64 consecutive attached elements OF ONE BODY (row_layout.hpp's block_row over total, a body being
//                           a row).  Every load first (idx, w2, active, u, z, then the
//                           node's x), then attach.hpp's six terms about rec[body].c, folded by track_block_sum -- the butterfly of
//                           entry_partial_block and the energies -- into partial [6][n_part]; the block's number of active elements by
//                           __popcll(__ballot) into cnt [n_part].  Every lane stays: one beyond the body's elements adds six +0.0.
//   attach_reduce_kernel    one workgroup per (body, component): entry_reduce_row over the body's partials (energy_reduce_kernel's
//                           order) -> out [bodies][6]; then lane 0 adds that into the body's row of the contacts' sums rows [bodies][6]
//                           -- only where carry[body] != 0 -- and, for component 0, sums the blocks' active counts (the body's blocks by
//                           row_layout.hpp, ascending) into n_active [bodies]
// Every index is bounded: a block's slot < n_slots and a slot's body < n_bodies <= ADMM_MAX_SHAPES are checked before use; first + lane
// < n of the batch; a body's elements k < sum of total, the length of el_slot / el_elem; idx[e] is the batch's own device node id, as
// every local kernel reads it; blockIdx.x < n_part by the launch (the host counts the blocks from the same totals it uploads).
//
// Cost: tools/probe_attach.py prints the frame time with and without; DESIGN.md section 3 records what it printed (at most 0.15 ms per
// frame, an upper bound: the two runs are different scenes).  The three kernels move 48 B per element for the targets and 88 B per
// element for the load; the frame's added time is their three launches.
#pragma once
#include "kernels_rigid.hpp"
#include "attach.hpp"

namespace admm_dev {

struct AttachBatchDev { const int *idx; const double *w2; const int *active; const double *u, *z; double *targets; const double *local; int n, body; };
struct AttachBlock { int slot, first; };

__global__ __launch_bounds__(ENERGY_BLOCK) void attach_targets_kernel(const AttachBlock *__restrict__ blk, const AttachBatchDev *__restrict__ bat, const int n_slots, const int n_bodies,
                                                                      const admm_rigid::Record *__restrict__ rec) {
    const AttachBlock B = blk[blockIdx.x];
    if (B.slot < 0 || B.slot >= n_slots) return;
    const AttachBatchDev A = bat[B.slot];
    const int e = B.first + (int)threadIdx.x;
    if (A.body < 0 || A.body >= n_bodies || e < 0 || e >= A.n) return;
    double c[3], R[9], r[3], t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { c[j] = rec[A.body].c[j]; r[j] = A.local[3 * (size_t)e + j]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rec[A.body].R[k];
    admm_attach::target(c, R, r, t);
#pragma unroll
    for (int j = 0; j < 3; ++j) A.targets[3 * (size_t)e + j] = t[j];
}

__global__ __launch_bounds__(ENERGY_BLOCK) void attach_partial_kernel(const int *__restrict__ el_slot, const int *__restrict__ el_elem, const AttachBatchDev *__restrict__ bat, const int n_slots,
                                                                      const int n_bodies, const long long *__restrict__ total, const admm_rigid::Record *__restrict__ rec,
                                                                      const double *__restrict__ x, const int n_part, double *__restrict__ partial, int *__restrict__ cnt) {
    long long base, blk0;
    const int body = admm_layout::block_row(total, n_bodies, blockIdx.x, base, blk0);
    if (body < 0) return;                   // beyond the last body's blocks: nobody reads this partial
    const long long r = ((long long)blockIdx.x - blk0) * ENERGY_BLOCK + threadIdx.x;
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int act = 0;
    if (r < total[body]) {
        const int s = el_slot[base + r], e = el_elem[base + r];
        if (s >= 0 && s < n_slots) {
            const AttachBatchDev A = bat[s];
            if (e >= 0 && e < A.n) {
                // every load first: the element's own rows, then its node's position
                const size_t n = (size_t)A.n;
                const int id = A.idx[e];
                const double w2 = A.w2[e];
                act = A.active[e];
                double U[3], Z[3], X[3], pivot[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) { U[j] = A.u[(size_t)j * n + e]; Z[j] = A.z[(size_t)j * n + e]; pivot[j] = rec[body].c[j]; }
#pragma unroll
                for (int j = 0; j < 3; ++j) X[j] = x[3 * (size_t)id + j];
                admm_attach::load_terms(act, w2, U, Z, X, pivot, t);
            }
        }
    }
    const unsigned long long m = __ballot(act != 0);
#pragma unroll
    for (int q = 0; q < 6; ++q) track_block_sum(t[q], &partial[(size_t)q * n_part + blockIdx.x]);
    if (threadIdx.x == 0) cnt[blockIdx.x] = __popcll(m);
}

// workgroup (body, component) = (blockIdx.x / 6, blockIdx.x % 6) -> out[body][component]; rows: the contacts' sums (rigid_reduce_kernel)
__global__ __launch_bounds__(ENERGY_REDUCE) void attach_reduce_kernel(const long long *__restrict__ total, const int *__restrict__ carry, const int n_part, const double *__restrict__ partial,
                                                                      const int *__restrict__ cnt, double *__restrict__ out, long long *__restrict__ n_active, double *__restrict__ rows) {
    const int b = (int)blockIdx.x / 6, comp = (int)blockIdx.x % 6;
    entry_reduce_row(b, comp, total, n_part, partial, &out[(size_t)b * 6 + comp]);
    if (threadIdx.x != 0) return;
    if (carry[b] != 0) rows[(size_t)b * 6 + comp] = admm_attach::combine(rows[(size_t)b * 6 + comp], out[(size_t)b * 6 + comp]);
    if (comp == 0) {
        const long long blk0 = admm_layout::blocks_before(total, b), nb = admm_layout::row_blocks(total[b]);
        long long na = 0;
        for (long long i = 0; i < nb; ++i) na += cnt[blk0 + i];      // ascending block
        n_active[b] = na;
    }
}

} // namespace admm_dev
