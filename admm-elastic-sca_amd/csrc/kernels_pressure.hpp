// kernels_pressure.hpp -- the pressure chambers of pressure.hpp on the device: per chamber the volume, area and area vector of its
// oriented triangles at the frame-start x, the pressure its law gives, and dt f / m added to v.  Extension, no reference counterpart;
// admm_hip_step launches it after the body surfaces' update and the side latch and before the prologue (or the ordered explicit list),
// and only when some chamber is active; admm_hip_get_chamber_state runs the first two stages for one chamber on demand.  No atomics
// anywhere: the same state gives the same bits.
//
// All chambers of a context go through ONE launch per stage, as the damping groups do (kernels_damping.hpp):
//   pressure_terms_kernel    a block -> (chamber, first triangle) table built at finalize gives every one-wave block of 64 lanes 64
//                            consecutive triangles of one chamber, counted from the chamber's first; the lane's triangle holds the device
//                            positions of its nodes (mapped through iperm at upload).  It stores the normal n = a x b [3][triangles] and one
//                            partial per block and term (track_block_sum).  A lane beyond its chamber, or of a chamber the launch passes
//                            over, returns before its first load of the state.
//   pressure_reduce_kernel   one workgroup of 256 per chamber: the partials of its blocks in energy_reduce_kernel's order, the five terms
//                            side by side; applies the law and writes the chamber's record; `count` adds a collapse to the chamber's counter
//   pressure_apply_kernel    one thread per distinct chamber node (caller's order): walks the node's corners through a node CSR ordered by
//                            chamber, triangle, corner, skipping inactive chambers, f = f + p (n / 6), then v <- v + (dt f) / m from d_m3.
//                            A node none of whose chambers is active is not written.
// `all` = 0: the frame's launch, active chambers only; 1: the on-demand state, every chamber of the launch.
//
// Bound by memory and small: per triangle 12 B of positions' indices, 72 B of x gathered in 24-byte runs, 24 B of normal written; per
// node corner 12 B of CSR, 4 B of chamber, 24 B of normal read.
#pragma once
#include "kernels_energy.hpp"
#include "pressure.hpp"

namespace admm_dev {

constexpr int PRES_BLOCK = admm_pressure::SUM_BLOCK, PRES_REDUCE = admm_pressure::SUM_REDUCE, PRES_APPLY = 256;
static_assert(PRES_BLOCK == ENERGY_BLOCK && PRES_REDUCE == ENERGY_REDUCE, "pressure.hpp restates the sums of kernels_energy.hpp");

struct PresBlock { int chamber, first; };                            // a block's chamber and its first triangle (index into all triangles)
struct PresChamber { int tri_first, n_tris, blk_first, n_blk, origin, pad_; };   // origin: device position of the first triangle's first node
struct PresLaw { double par0, par1; int mode, active; };             // written by pressure_set_law_kernel from kernel arguments

struct PresDev {
    const PresBlock *blocks;      // [all blocks]
    const PresChamber *chambers;  // [chambers]
    const PresLaw *law;           // [chambers]
    const int *tri;               // [all triangles][3] device positions of the corners
    const int *tri_chamber;       // [all triangles]
    admm_pressure::Record *rec;   // [chambers]
    long long *collapsed;         // [chambers] frames of a gas chamber whose volume was not positive and finite
    double *nrm;                  // [3][all triangles]
    double *part;                 // [N_SUMS][n_blocks_total]
    int n_blocks_total, n_tris_total;
    // the gather: node k of the distinct chamber nodes sits at device position node[k] and owns the corners ptr[k] .. ptr[k + 1): the
    // corner's triangle is off[e] (node_csr.hpp: row j of its normal at nrm[off + j * stride])
    const int *node, *ptr; const long long *off; const int *stride; int n_nodes;
};

__global__ __launch_bounds__(PRES_BLOCK) void pressure_set_law_kernel(PresLaw *__restrict__ law, const int c, const int mode, const double par0, const double par1, const int active) {
    if (threadIdx.x == 0) { law[c].par0 = par0; law[c].par1 = par1; law[c].mode = mode; law[c].active = active; }
}

// blk0: the launch's first block in the table
__global__ __launch_bounds__(PRES_BLOCK) void pressure_terms_kernel(const PresDev d, const int blk0, const int all, const double *__restrict__ x) {
    const int blk = blk0 + (int)blockIdx.x;
    const PresBlock B = d.blocks[blk];
    if (!all && !d.law[B.chamber].active) return;
    const PresChamber C = d.chambers[B.chamber];
    const int t = B.first + (int)threadIdx.x;
    if (t >= C.tri_first + C.n_tris) return;
    const size_t po = 3 * (size_t)C.origin, p0 = 3 * (size_t)d.tri[3 * (size_t)t], p1 = 3 * (size_t)d.tri[3 * (size_t)t + 1], p2 = 3 * (size_t)d.tri[3 * (size_t)t + 2];
    const double o[3] = {x[po], x[po + 1], x[po + 2]}, x0[3] = {x[p0], x[p0 + 1], x[p0 + 2]}, x1[3] = {x[p1], x[p1 + 1], x[p1 + 2]}, x2[3] = {x[p2], x[p2 + 1], x[p2 + 2]};
    double n[3], s[admm_pressure::N_SUMS];
    admm_pressure::tri_terms(o, x0, x1, x2, n, s);
#pragma unroll
    for (int j = 0; j < 3; ++j) d.nrm[(size_t)j * d.n_tris_total + t] = n[j];
#pragma unroll
    for (int q = 0; q < admm_pressure::N_SUMS; ++q) track_block_sum(s[q], &d.part[(size_t)q * d.n_blocks_total + blk]);
}

// one workgroup per chamber (c0 + blockIdx.x): its blocks' partials -> the five sums, the law, the record
__global__ __launch_bounds__(PRES_REDUCE) void pressure_reduce_kernel(const PresDev d, const int c0, const int all, const int count) {
    constexpr int NT = admm_pressure::N_SUMS;
    __shared__ double acc[NT][PRES_REDUCE];
    const int c = c0 + (int)blockIdx.x, t = threadIdx.x;
    const PresLaw W = d.law[c];
    if (!all && !W.active) return;      // (uniform over the workgroup)
    const PresChamber C = d.chambers[c];
    double a[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) a[q] = 0.0;
    for (int i = t; i < C.n_blk; i += PRES_REDUCE) {
#pragma unroll
        for (int q = 0; q < NT; ++q) a[q] += d.part[(size_t)q * d.n_blocks_total + C.blk_first + i];
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q][t] = a[q];
    __syncthreads();
    for (int h = PRES_REDUCE / 2; h >= 1; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int q = 0; q < NT; ++q) acc[q][t] += acc[q][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        double sum[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) sum[q] = acc[q][0];
        admm_pressure::Record R;
        const int collapsed = admm_pressure::finish(sum, W.mode, W.par0, W.par1, R);
        long long n = d.collapsed[c];
        if (count && collapsed) { n += 1; d.collapsed[c] = n; }
        R.n_tris = C.n_tris; R.collapsed = n;
        d.rec[c] = R;
    }
}

__global__ __launch_bounds__(PRES_APPLY) void pressure_apply_kernel(const PresDev d, const double dt, const double *__restrict__ m3, double *__restrict__ v) {
    const int k = (int)blockIdx.x * PRES_APPLY + (int)threadIdx.x;
    if (k >= d.n_nodes) return;
    double f[3] = {0.0, 0.0, 0.0};
    bool any = false;
    for (int e = d.ptr[k]; e < d.ptr[k + 1]; ++e) {
        const long long t = d.off[e];
        const int c = d.tri_chamber[t];
        if (!d.law[c].active) continue;
        any = true;
        const size_t st = (size_t)d.stride[e];
        const double n[3] = {d.nrm[t], d.nrm[t + st], d.nrm[t + 2 * st]};
        admm_pressure::add_corner(d.rec[c].pressure, n, f);
    }
    if (!any) return;
    const size_t p = 3 * (size_t)d.node[k];
    double dv[3];
    admm_pressure::increment(dt, f, m3[p], dv);
    v[p] = v[p] + dv[0]; v[p + 1] = v[p + 1] + dv[1]; v[p + 2] = v[p + 2] + dv[2];
}

} // namespace admm_dev
