// kernels_reaction.hpp -- the reactions of reaction.hpp evaluated on the device: per COLLISION / ANCHOR element the force its constraint
// exerted on its node in the last frame and its depth, the nodes' sums in the caller's node order, the compact list of the nodes in
// contact and their resultant.  Extension, no reference counterpart; no product path launches any of this unless the caller asks
// (admm_hip_batch_reaction, admm_hip_node_reactions, admm_hip_get_contacts, admm_hip_contact_resultant).  Everything reads u, z, x and
// writes buffers of its own; no atomics anywhere: two calls on the same state give the same bits.
//
// reaction_elem_kernel, one lane per element, ENERGY_BLOCK = 64-element blocks: reads w2[e], the element's u and z (SoA [3][n], coalesced)
// and its node's x (gathered through idx) and writes seven rows of SoA [7][n]: f0 f1 f2, depth, z0 z1 z2 (the point: a copy, so that
// the gather reads one buffer with one stride).  A lane beyond the batch returns before its first load.
//
// reaction_gather_kernel, one lane per node in the CALLER's node order: two CSRs built on the host at first use (0: the collision
// batches, 1: the anchor batches), entries in batch order, then local element order.  Per CSR the lane adds its entries' forces
// sequentially, s = 0.0; s = s + v.  Over the collision entries it also keeps the node's depth and point: depth = 0.0, point = 0; an entry
// with d > depth replaces both (the largest depth; ties and d = 0 keep the earlier one; a NaN depth never wins).  Output, one buffer:
// f_contact [n][3], f_anchor [n][3], depth [n], point [n][3].  A node with no element gets exactly 0.0 everywhere.
//
// Two pieces are written once and shared by this file, kernels_surface_reaction.hpp, kernels_rigid.hpp and kernels_attach.hpp:
//   wave_scan_inclusive / wave_scan_row   the 64-lane shuffle scan (no LDS, no barrier) and, over it, the exclusive scan of one row of
//                           block counts by ONE wave, chunk after chunk of 64 in ascending order with a running carry -> offsets, total.
//                           row_scan_kernel runs it with one wave per row of a [rows][n_blocks] table
//   contact_slot            the compaction's prologue, called by every lane of the workgroup before any early return (it holds a
//                           __ballot and a __syncthreads): a node's flag depth > depth_min, its depth and its place = its block's
//                           offset + the counts of the waves before its own (LDS) + __popcll(ballot & lanes below)
// Where the 64-contact blocks of several rows sit is row_layout.hpp's rule, not restated here.
//
// Compaction of the nodes with depth > depth_min, in ascending node index, three launches and no spinning across workgroups:
//   contact_count_kernel    RX_BLOCK = 128 nodes per block (two waves): contact_slot's flags, one count per block
//   row_scan_kernel         one row, ONE workgroup of RX_SCAN = 64 lanes: block offsets and the total, which stays on the device
//   contact_scatter_kernel  contact_slot again, now with the offsets; writes the 64-byte record when the place is below `capacity`
// The resultant of all contacts is the per-entry sum below with ONE row: entry_partial_kernel with total = the contacts' count and no
// permutation (contact k is record k), then entry_reduce_kernel -- the fixed-order two-stage sum of kernels_energy.hpp, restated in
// reaction.hpp.  The second stage adds the ceil(count / 64) partials that are filled; reaction.hpp's last paragraph says why reducing
// over more, trailing +0.0 partials gives the same bits.
//
// Cost: not measured, no timing claimed.  Expected to be bound by memory: an element reads 84 B (idx, w2, u, z, its node's x) and writes
// 56 B; a node's gather reads its CSR bounds, a 12 B entry and 56 B per incident element and writes 80 B; the count reads 8 B per node,
// the scatter 64 B per node in contact and writes as much.
//
// Contact attribution (attribution.hpp; admm_hip_get_contact_owners, admm_hip_entry_resultants; only while the switch is on).  None of the
// kernels above changes or is launched differently; these run behind them, no atomics, fixed orders:
//   contact_owner_scatter_kernel  contact_slot's flags and places again; a node in contact walks its collision entries by the
//                           gather's rule (the largest depth, the first on ties) and takes the winning element's owner and normal from the
//                           record form 8 wrote, then splits the node's f_contact about that normal: one 64-byte OwnerRecord per contact
//   entry_count_kernel      one wave per ENERGY_BLOCK = 64 contacts k < count: per row q (an entry of the list, the last row: owner -1) the
//                           number of the block's contacts with that entry, by __popcll(__ballot)
//   row_scan_kernel         one wave per row: the row's block counts -> block offsets and the row's total
//   entry_place_kernel      the count kernel's flags again: perm[(the totals of the rows before) + block offset + rank in the wave] = k, the
//                           contacts sorted by row, ascending k inside a row
//   entry_partial_kernel    one wave per 64 consecutive contacts OF ONE ROW (a block finds its row from the totals: row_layout.hpp's
//                           block_row): the six terms of reaction.hpp summed by track_block_sum, the row's last block padded with +0.0
//   entry_reduce_kernel     one workgroup per (row, component): the row's partials in energy_reduce_kernel's order -- so a row is exactly the
//                           two-stage sum of reaction.hpp over the contacts with that entry
#pragma once
#include "kernels_energy.hpp"
#include "reaction.hpp"
#include "attribution.hpp"
#include "row_layout.hpp"

namespace admm_dev {

constexpr int RX_BLOCK = 128, RX_WAVES = RX_BLOCK / 64, RX_SCAN = 64;
constexpr int RX_ROWS = 7;      // rows of the element buffer: f0 f1 f2, depth, z0 z1 z2
static_assert(admm_reaction::RESULTANT_BLOCK == ENERGY_BLOCK && admm_reaction::RESULTANT_REDUCE == ENERGY_REDUCE, "reaction.hpp restates the sums of kernels_energy.hpp");
static_assert(RX_SCAN == 64, "wave_scan_row is a one-wave shuffle scan");
static_assert(admm_layout::ROW_BLOCK == ENERGY_BLOCK, "row_layout.hpp cuts the rows into the blocks track_block_sum sums");

struct ContactRecord { int node; int pad_; double f[3], point[3], depth; };      // = admm_hip_contact
static_assert(sizeof(ContactRecord) == 64, "the record is 64 bytes");

__global__ __launch_bounds__(ENERGY_BLOCK) void reaction_elem_kernel(const int n, const int *__restrict__ idx, const double *__restrict__ w2, const double *__restrict__ u,
                                                                     const double *__restrict__ z, const double *__restrict__ x, double *__restrict__ out) {
    const int e = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int id = idx[e];
    double U[3], Z[3], X[3], f[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { U[j] = u[(size_t)j * n + e]; Z[j] = z[(size_t)j * n + e]; X[j] = x[3 * (size_t)id + j]; }
    admm_reaction::force(w2[e], U, Z, X, f);
    const double d = admm_reaction::depth(U);
#pragma unroll
    for (int j = 0; j < 3; ++j) { out[(size_t)j * n + e] = f[j]; out[(size_t)(4 + j) * n + e] = Z[j]; }
    out[(size_t)3 * n + e] = d;
}

// entry k of a CSR: row r of its element at el[off[k] + r stride[k]]
__global__ __launch_bounds__(ENERGY_BLOCK) void reaction_gather_kernel(const int n_nodes, const int *__restrict__ ptr_c, const long long *__restrict__ off_c, const int *__restrict__ stride_c,
                                                                       const int *__restrict__ ptr_a, const long long *__restrict__ off_a, const int *__restrict__ stride_a,
                                                                       const double *__restrict__ el, double *__restrict__ out) {
    const int i = (int)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    const size_t n = (size_t)n_nodes;
    double s[3] = {0.0, 0.0, 0.0}, depth = 0.0, pt[3] = {0.0, 0.0, 0.0};
    for (int k = ptr_c[i], k1 = ptr_c[i + 1]; k < k1; ++k) {
        const double *p = el + off_c[k];
        const size_t st = (size_t)stride_c[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] = s[j] + p[j * st];
        const double d = p[3 * st];
        if (d > depth) { depth = d; pt[0] = p[4 * st]; pt[1] = p[5 * st]; pt[2] = p[6 * st]; }
    }
    double a[3] = {0.0, 0.0, 0.0};
    for (int k = ptr_a[i], k1 = ptr_a[i + 1]; k < k1; ++k) {
        const double *p = el + off_a[k];
        const size_t st = (size_t)stride_a[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] = a[j] + p[j * st];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) { out[3 * (size_t)i + j] = s[j]; out[3 * n + 3 * (size_t)i + j] = a[j]; out[7 * n + 3 * (size_t)i + j] = pt[j]; }
    out[6 * n + i] = depth;
}

// ---- the shared pieces: one wave scan, one compaction prologue ------------------------------------------------------------------------
// inclusive scan of v over the 64 lanes of a wave: a shuffle ladder, no LDS, no barrier
__device__ __forceinline__ int wave_scan_inclusive(int v, const int lane) {
#pragma unroll
    for (int d = 1; d < RX_SCAN; d <<= 1) { const int o = __shfl_up(v, d, RX_SCAN); if (lane >= d) v += o; }
    return v;
}

// one wave: exclusive scan of cnt[0 .. n_blocks) -> off, chunk after chunk of 64 in ascending order with a running carry; -> the total
// (uniform: every lane runs every chunk)
__device__ __forceinline__ int wave_scan_row(const int n_blocks, const int *__restrict__ cnt, int *__restrict__ off) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n_blocks; base += RX_SCAN) {
        const int i = base + lane;
        const int v = i < n_blocks ? cnt[i] : 0;
        const int incl = wave_scan_inclusive(v, lane);
        if (i < n_blocks) off[i] = carry + incl - v;
        carry += __shfl(incl, RX_SCAN - 1, RX_SCAN);
    }
    return carry;
}

// row blockIdx.x of blk_count [rows][n_blocks]: wave_scan_row -> blk_off, total[row]; one wave per row (the compaction: one row)
__global__ __launch_bounds__(RX_SCAN) void row_scan_kernel(const int n_blocks, const int *__restrict__ blk_count, int *__restrict__ blk_off, long long *__restrict__ total) {
    const int t = wave_scan_row(n_blocks, blk_count + (size_t)blockIdx.x * n_blocks, blk_off + (size_t)blockIdx.x * n_blocks);
    if (threadIdx.x == 0) total[blockIdx.x] = t;
}

// The compaction's prologue for node blockIdx.x RX_BLOCK + threadIdx.x.  It holds a __ballot and a __syncthreads: EVERY lane of the
// workgroup calls it, before any early return.  in: the node is in contact (depth > depth_min); place: blk_off's offset of the block (0
// without blk_off) + the counts of the waves before the node's own + the lanes in contact below it; block_count: the block's nodes in contact
struct ContactSlot { bool in; double depth; long long place; int block_count; };
__device__ __forceinline__ ContactSlot contact_slot(const int n_nodes, const double *__restrict__ depth, const double depth_min, const int *__restrict__ blk_off) {
    __shared__ int wave_count[RX_WAVES];
    const int i = (int)blockIdx.x * RX_BLOCK + threadIdx.x;
    ContactSlot s;
    s.depth = i < n_nodes ? depth[i] : 0.0;
    s.in = i < n_nodes && admm_reaction::in_contact(s.depth, depth_min);
    const unsigned long long m = __ballot(s.in);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    s.place = (blk_off ? blk_off[blockIdx.x] : 0) + __popcll(m & ((1ull << lane) - 1ull));
    s.block_count = 0;
    for (int w = 0; w < RX_WAVES; ++w) { if (w < wave) s.place += wave_count[w]; s.block_count += wave_count[w]; }
    return s;
}

// depth [n_nodes] -> one count per RX_BLOCK nodes
__global__ __launch_bounds__(RX_BLOCK) void contact_count_kernel(const int n_nodes, const double *__restrict__ depth, const double depth_min, int *__restrict__ blk_count) {
    const ContactSlot s = contact_slot(n_nodes, depth, depth_min, nullptr);
    if (threadIdx.x == 0) blk_count[blockIdx.x] = s.block_count;
}

// the records of the nodes in contact, ascending node index, from the gather's output `nodes` (its layout); places >= capacity are dropped
__global__ __launch_bounds__(RX_BLOCK) void contact_scatter_kernel(const int n_nodes, const double *__restrict__ nodes, const double depth_min, const int *__restrict__ blk_off,
                                                                   const long long capacity, ContactRecord *__restrict__ rec) {
    const size_t n = (size_t)n_nodes;
    const ContactSlot s = contact_slot(n_nodes, nodes + 6 * n, depth_min, blk_off);
    if (!s.in || s.place >= capacity) return;
    const int i = (int)blockIdx.x * RX_BLOCK + threadIdx.x;
    ContactRecord r;
    r.node = i; r.pad_ = 0; r.depth = s.depth;
#pragma unroll
    for (int j = 0; j < 3; ++j) { r.f[j] = nodes[3 * (size_t)i + j]; r.point[j] = nodes[7 * n + 3 * (size_t)i + j]; }
    rec[s.place] = r;
}

// ---- contact attribution ------------------------------------------------------------------------------------------------------------
struct OwnerRecord { int node; int entry; double normal[3], f_normal, f_tangent[3]; };      // = admm_hip_contact_owner
static_assert(sizeof(OwnerRecord) == 64, "the record is 64 bytes");

// el, ptr_c / off_c / stride_c: the gather's element buffer and its collision CSR; at_idx[k]: where entry k's element sits in owner and in
// every row of normal (SoA [3][at_stride])
__global__ __launch_bounds__(RX_BLOCK) void contact_owner_scatter_kernel(const int n_nodes, const double *__restrict__ nodes, const double depth_min, const int *__restrict__ blk_off,
                                                                         const long long capacity, const int *__restrict__ ptr_c, const long long *__restrict__ off_c,
                                                                         const int *__restrict__ stride_c, const long long *__restrict__ at_idx, const double *__restrict__ el,
                                                                         const int *__restrict__ owner, const double *__restrict__ normal, const long long at_stride,
                                                                         OwnerRecord *__restrict__ rec) {
    const ContactSlot s = contact_slot(n_nodes, nodes + 6 * (size_t)n_nodes, depth_min, blk_off);
    if (!s.in || s.place >= capacity) return;
    const int i = (int)blockIdx.x * RX_BLOCK + threadIdx.x;
    double depth = 0.0;
    int win = -1;      // (a node in contact has an entry with d > 0)
    for (int k = ptr_c[i], k1 = ptr_c[i + 1]; k < k1; ++k) {
        const double dk = el[off_c[k] + 3 * (size_t)stride_c[k]];
        if (dk > depth) { depth = dk; win = k; }
    }
    OwnerRecord r;
    r.node = i; r.entry = -1; r.normal[0] = r.normal[1] = r.normal[2] = 0.0;
    if (win >= 0) {
        const long long a = at_idx[win];
        r.entry = owner[a];
#pragma unroll
        for (int j = 0; j < 3; ++j) r.normal[j] = normal[(size_t)j * (size_t)at_stride + a];
    }
    const double f[3] = {nodes[3 * (size_t)i], nodes[3 * (size_t)i + 1], nodes[3 * (size_t)i + 2]};
    admm_attribution::split(f, r.normal, r.f_normal, r.f_tangent);
    rec[s.place] = r;
}

// the row of contact k: its entry, the last row n_rows - 1 for owner -1 (and for an entry beyond the list, which the record cannot hold)
__device__ __forceinline__ int entry_row(const OwnerRecord *__restrict__ rec, const long long k, const int n_rows) {
    const int q = rec[k].entry;
    return (q >= 0 && q < n_rows - 1) ? q : n_rows - 1;
}

// blk_count [n_rows][n_blocks]
__global__ __launch_bounds__(ENERGY_BLOCK) void entry_count_kernel(const long long *__restrict__ count, const OwnerRecord *__restrict__ rec, const int n_rows, const int n_blocks,
                                                                   int *__restrict__ blk_count) {
    const long long k = (long long)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    const int row = k < *count ? entry_row(rec, k, n_rows) : -1;
    for (int q = 0; q < n_rows; ++q) {      // (uniform: every lane runs every row)
        const unsigned long long m = __ballot(row == q);
        if (threadIdx.x == 0) blk_count[(size_t)q * n_blocks + blockIdx.x] = __popcll(m);
    }
}

// perm [count]: the contacts sorted by row
__global__ __launch_bounds__(ENERGY_BLOCK) void entry_place_kernel(const long long *__restrict__ count, const OwnerRecord *__restrict__ rec, const int n_rows, const int n_blocks,
                                                                   const int *__restrict__ blk_off, const long long *__restrict__ total, int *__restrict__ perm) {
    const long long k = (long long)blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    const int row = k < *count ? entry_row(rec, k, n_rows) : -1;
    long long base = 0;
    for (int q = 0; q < n_rows; ++q) {
        const unsigned long long m = __ballot(row == q);
        if (row == q) perm[base + blk_off[(size_t)q * n_blocks + blockIdx.x] + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = (int)k;
        base += total[q];
    }
}

// block blockIdx.x, which row_layout.hpp's block_row placed in a row of row_total contacts behind `base` contacts and blk0 blocks: the
// six terms of reaction.hpp about `pivot`, summed by track_block_sum -> partial [6][n_part] at blockIdx.x; perm null: contact k is record k
// (shared by entry_partial_kernel and kernels_rigid.hpp's rigid_partial_kernel)
__device__ __forceinline__ void entry_partial_block(const ContactRecord *__restrict__ rec, const int *__restrict__ perm, const long long row_total, const long long base, const long long blk0,
                                                    const double *pivot, const int n_part, double *__restrict__ partial) {
    const long long r = ((long long)blockIdx.x - blk0) * ENERGY_BLOCK + threadIdx.x;
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (r < row_total) {
        const ContactRecord c = rec[perm ? perm[base + r] : (int)(base + r)];
        admm_reaction::resultant_terms(c.f, c.point, pivot, t);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) track_block_sum(t[q], &partial[(size_t)q * n_part + blockIdx.x]);
}

// partial [6][n_part]: block B is block B - (the blocks of the rows before) of its row.  One row, total = the contacts' count and no perm:
// the resultant of all contacts (admm_hip_contact_resultant)
__global__ __launch_bounds__(ENERGY_BLOCK) void entry_partial_kernel(const ContactRecord *__restrict__ rec, const int *__restrict__ perm, const int n_rows, const long long *__restrict__ total,
                                                                     const double p0, const double p1, const double p2, const int n_part, double *__restrict__ partial) {
    long long base, blk0;
    const int row = admm_layout::block_row(total, n_rows, blockIdx.x, base, blk0);      // (uniform across the block)
    if (row < 0) return;                    // beyond the last row's blocks: nobody reads this partial
    const double pivot[3] = {p0, p1, p2};
    entry_partial_block(rec, perm, total[row], base, blk0, pivot, n_part, partial);
}

// one (row, component) by the whole workgroup: the row's partials in energy_reduce_kernel's order -> *out
// (shared by entry_reduce_kernel and kernels_rigid.hpp's rigid_reduce_kernel)
__device__ __forceinline__ void entry_reduce_row(const int row, const int comp, const long long *__restrict__ total, const int n_part, const double *__restrict__ partial, double *__restrict__ out) {
    __shared__ double acc[ENERGY_REDUCE];
    const int t = threadIdx.x;
    const int n = (int)admm_layout::row_blocks(total[row]);
    const double *p = partial + (size_t)comp * n_part + admm_layout::blocks_before(total, row);
    double a = 0.0;
    for (int i = t; i < n; i += ENERGY_REDUCE) a += p[i];
    acc[t] = a;
    __syncthreads();
    for (int h = ENERGY_REDUCE / 2; h >= 1; h >>= 1) {
        if (t < h) acc[t] += acc[t + h];
        __syncthreads();
    }
    if (t == 0) *out = acc[0];
}

// workgroup (row, component) = (blockIdx.x / 6, blockIdx.x % 6): out[row][component], energy_reduce_kernel's order over the row's partials
__global__ __launch_bounds__(ENERGY_REDUCE) void entry_reduce_kernel(const int n_rows, const long long *__restrict__ total, const int n_part, const double *__restrict__ partial,
                                                                     double *__restrict__ out) {
    const int row = (int)blockIdx.x / 6, comp = (int)blockIdx.x % 6;
    entry_reduce_row(row, comp, total, n_part, partial, &out[(size_t)row * 6 + comp]);
}

} // namespace admm_dev
