// kernels_damping.hpp -- the velocity filter of damping.hpp on the device: per damping group the mass, centre of mass, momentum, angular
// momentum and inertia tensor of its nodes, the angular velocity, and the damped velocities written back into v.  Extension, no
// reference counterpart; admm_hip_step launches it directly after epilogue_kernel, and only when some group has a rate above zero;
// admm_hip_get_group_moments runs the first four stages for one group on demand.  No atomics anywhere: the same state gives the same bits.
//
// All groups of a context go through ONE launch per stage.  A block -> (group, first node) table built at finalize gives every one-wave
// block of 64 lanes 64 consecutive nodes of one group, counted from the group's first node; the lane's node in the caller's order goes
// through iperm to its device position, as in energy_node_kernel.  A lane beyond its group, or of a group the launch passes over,
// returns before its first load of the state.
//   damping_pass1_kernel    m, x, v of the node -> the eight terms of node_terms_1, one partial per block and term (track_block_sum)
//   damping_reduce1_kernel  one workgroup of 256 per group: the partials of its blocks in energy_reduce_kernel's order (thread t adds
//                           partials t, t + 256, ... ascending, then the LDS fold), all eight terms side by side; forms c, v_c
//   damping_pass2_kernel    the nine terms of node_terms_2 about c, v_c
//   damping_reduce2_kernel  likewise; solves omega, completes the group's moments record
//   damping_apply_kernel    v <- v + beta ((v_c + omega x r) - v) for groups with internal > 0, then v <- s v
// Five launches per frame when any group has internal > 0, one (apply) otherwise.  `which` selects the groups a pass covers: a group's
// mode is 0 (both rates zero: untouched), 1 (drag only: apply alone) or 2 (internal > 0); the passes and reductions take groups with
// mode >= `which_min`, and with which_min = 0 every group of the launch (the on-demand moments).
//
// Streaming and bound by memory: per pass a node reads its iperm entry (4 B), its mass (8 B of the 24 B of m3 it sits in), x and v (48 B);
// the apply reads the same and writes v (24 B).  The gathers through iperm are 24-byte runs at scattered device positions.
#pragma once
#include "kernels_energy.hpp"
#include "damping.hpp"

namespace admm_dev {

constexpr int DAMP_BLOCK = admm_damping::SUM_BLOCK, DAMP_REDUCE = admm_damping::SUM_REDUCE;
static_assert(DAMP_BLOCK == ENERGY_BLOCK && DAMP_REDUCE == ENERGY_REDUCE, "damping.hpp restates the sums of kernels_energy.hpp");

struct DampBlock { int group, first; };                               // a block's group and its first node (caller's order)
struct DampGroup { int node_first, node_count, blk_first, n_blk; };   // a group's node range and its run of blocks
struct DampRate { double beta, s; int mode, pad_; };                  // mode 0: untouched, 1: drag only, 2: internal (and drag)

struct DampDev {
    const DampBlock *blocks;      // [all blocks]
    const DampGroup *groups;      // [groups]
    const DampRate *rate;         // [groups]
    admm_damping::Moments *mom;   // [groups]
    double *vc;                   // [groups][3]
    double *part;                 // [N_SUMS_2][n_blocks_total]: a stage's partials (pass 1 uses the first eight rows)
    int n_blocks_total;
};

__global__ __launch_bounds__(DAMP_BLOCK) void damping_set_rate_kernel(DampRate *__restrict__ rate, const int g, const double beta, const double s, const int mode) {
    if (threadIdx.x == 0) { rate[g].beta = beta; rate[g].s = s; rate[g].mode = mode; rate[g].pad_ = 0; }
}

// PASS 1: node_terms_1, 2: node_terms_2.  blk0: the launch's first block in the table.
template <int PASS>
__global__ __launch_bounds__(DAMP_BLOCK) void damping_pass_kernel(const DampDev d, const int blk0, const int which_min, const int *__restrict__ iperm, const double *__restrict__ m3,
                                                                  const double *__restrict__ x, const double *__restrict__ v) {
    const int blk = blk0 + (int)blockIdx.x;
    const DampBlock B = d.blocks[blk];
    if (d.rate[B.group].mode < which_min) return;
    const DampGroup G = d.groups[B.group];
    const int i = B.first + (int)threadIdx.x;
    if (i >= G.node_first + G.node_count) return;
    const size_t p = 3 * (size_t)iperm[i];
    const double m = m3[p];
    const double X[3] = {x[p], x[p + 1], x[p + 2]}, V[3] = {v[p], v[p + 1], v[p + 2]};
    constexpr int NT = PASS == 1 ? admm_damping::N_SUMS_1 : admm_damping::N_SUMS_2;
    double t[NT];
    if (PASS == 1) admm_damping::node_terms_1(m, X, V, t);
    else {
        const admm_damping::Moments &R = d.mom[B.group];
        const double c[3] = {R.com[0], R.com[1], R.com[2]}, vc[3] = {d.vc[3 * B.group], d.vc[3 * B.group + 1], d.vc[3 * B.group + 2]};
        admm_damping::node_terms_2(m, X, V, c, vc, t);
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) track_block_sum(t[q], &d.part[(size_t)q * d.n_blocks_total + blk]);
}

// one workgroup per group (g0 + blockIdx.x): its blocks' partials -> the sums, in energy_reduce_kernel's order, then finish_1 / finish_2
template <int PASS>
__global__ __launch_bounds__(DAMP_REDUCE) void damping_reduce_kernel(const DampDev d, const int g0, const int which_min) {
    constexpr int NT = PASS == 1 ? admm_damping::N_SUMS_1 : admm_damping::N_SUMS_2;
    __shared__ double acc[NT][DAMP_REDUCE];
    const int g = g0 + (int)blockIdx.x, t = threadIdx.x;
    if (d.rate[g].mode < which_min) return;      // (uniform over the workgroup)
    const DampGroup G = d.groups[g];
    double a[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) a[q] = 0.0;
    for (int i = t; i < G.n_blk; i += DAMP_REDUCE) {
#pragma unroll
        for (int q = 0; q < NT; ++q) a[q] += d.part[(size_t)q * d.n_blocks_total + G.blk_first + i];
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q][t] = a[q];
    __syncthreads();
    for (int h = DAMP_REDUCE / 2; h >= 1; h >>= 1) {
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
        admm_damping::Moments &R = d.mom[g];      // (the record in place: pass 1 fills its first half, pass 2 the rest)
        double vc[3];
        if (PASS == 1) {
            R.n_nodes = G.node_count;
            admm_damping::finish_1(sum, R, vc);
            d.vc[3 * g] = vc[0]; d.vc[3 * g + 1] = vc[1]; d.vc[3 * g + 2] = vc[2];
        } else {
            vc[0] = d.vc[3 * g]; vc[1] = d.vc[3 * g + 1]; vc[2] = d.vc[3 * g + 2];
            admm_damping::finish_2(sum, vc, R);
        }
    }
}

__global__ __launch_bounds__(DAMP_BLOCK) void damping_apply_kernel(const DampDev d, const int *__restrict__ iperm, const double *__restrict__ x, double *__restrict__ v) {
    const int blk = (int)blockIdx.x;
    const DampBlock B = d.blocks[blk];
    const DampRate r = d.rate[B.group];
    if (r.mode == 0) return;
    const DampGroup G = d.groups[B.group];
    const int i = B.first + (int)threadIdx.x;
    if (i >= G.node_first + G.node_count) return;
    const size_t p = 3 * (size_t)iperm[i];
    double V[3] = {v[p], v[p + 1], v[p + 2]};
    if (r.mode == 2) {
        const admm_damping::Moments &R = d.mom[B.group];
        const double X[3] = {x[p], x[p + 1], x[p + 2]};
        const double c[3] = {R.com[0], R.com[1], R.com[2]}, om[3] = {R.omega[0], R.omega[1], R.omega[2]};
        const double vc[3] = {d.vc[3 * B.group], d.vc[3 * B.group + 1], d.vc[3 * B.group + 2]};
        admm_damping::apply_internal(r.beta, X, c, vc, om, V);
    }
    admm_damping::apply_drag(r.s, V);
    v[p] = V[0]; v[p + 1] = V[1]; v[p + 2] = V[2];
}

} // namespace admm_dev
