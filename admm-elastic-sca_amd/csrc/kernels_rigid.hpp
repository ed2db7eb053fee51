// kernels_rigid.hpp -- rigid bodies in the collision list, moved by their contacts (rigid.hpp): the device side.  Extension, no reference
// counterpart; no product path launches any of this unless a body is registered (admm_hip_add_rigid_body).  No atomics, fixed orders:
// two runs give the same bits.  All on the context's stream, eager, outside the captured graphs (abi_rigid.inc).
//
// The table: RigidTable { n, body_of_row[rows], K[bodies] } (the constants; uploaded by the host, accel rewritten by
// rigid_set_accel_kernel from kernel arguments) and rec [ADMM_MAX_SHAPES] admm_rigid::Record, the bodies' state and derived fields.
//
// Behind the frame's epilogue, after the reaction and attribution reports' launches and entry_count / row_scan / entry_place
// (kernels_reaction.hpp) have sorted the contacts by entry:
//   rigid_partial_kernel    entry_partial_kernel's block layout (row_layout.hpp's block_row) and entry_partial_block, the pivot of a row being its body's own centre
//                           rec[body].c (one read per block, uniform); a row that is no body returns before it writes
//   rigid_reduce_kernel     one workgroup per (body, component): entry_reduce_row over the body's row -> out [bodies][6]; a body's six
//                           sums are bit for bit the row admm_hip_entry_resultants(pivot = c) returns
//   rigid_integrate_kernel  ONE workgroup of 64 lanes, lane b < n: admm_rigid::step on rec[b] with its row and the row's contact count
// At the very start of the next step:
//   rigid_pose_kernel       ONE workgroup, lane b < n: admm_rigid::pose of rec[b] into the entry's par, frame, framed and motion of the
//                           shape table, by plain stores; nothing else of the table is written
// Every index is bounded: b < n <= ADMM_MAX_SHAPES, K[b].entry < shapes.n was checked at registration and a list of another length is
// refused while bodies exist; body_of_row is read at row < n_rows <= ADMM_MAX_SHAPES + 1.
//
// Cost: not measured here (tools/probe_rigid.py prints the frame time with and without).  The three kernels of this file move a few
// hundred bytes per body; the frame's added time is the reports' launches, about twenty short dependent kernels.
#pragma once
#include "kernels_reaction.hpp"
#include "rigid.hpp"

namespace admm_dev {

constexpr int RIGID_BLOCK = 64;
static_assert(ADMM_MAX_SHAPES <= RIGID_BLOCK, "one lane per body in one workgroup");

struct RigidTable { int n, pad_; int body_of_row[ADMM_MAX_SHAPES + 1]; int pad2_; admm_rigid::Const K[ADMM_MAX_SHAPES]; };

__global__ __launch_bounds__(ENERGY_BLOCK) void rigid_partial_kernel(const ContactRecord *__restrict__ rec, const int *__restrict__ perm, const int n_rows, const long long *__restrict__ total,
                                                                     const RigidTable *__restrict__ T, const admm_rigid::Record *__restrict__ body, const int n_part,
                                                                     double *__restrict__ partial) {
    long long base, blk0;
    const int row = admm_layout::block_row(total, n_rows, blockIdx.x, base, blk0);
    if (row < 0) return;
    const int b = T->body_of_row[row];
    if (b < 0) return;                      // not a rigid body: nobody reads this row's partials
    const double pivot[3] = {body[b].c[0], body[b].c[1], body[b].c[2]};
    entry_partial_block(rec, perm, total[row], base, blk0, pivot, n_part, partial);
}

// workgroup (body, component) = (blockIdx.x / 6, blockIdx.x % 6) -> out[body][component]
__global__ __launch_bounds__(ENERGY_REDUCE) void rigid_reduce_kernel(const RigidTable *__restrict__ T, const long long *__restrict__ total, const int n_part, const double *__restrict__ partial,
                                                                     double *__restrict__ out) {
    const int b = (int)blockIdx.x / 6, comp = (int)blockIdx.x % 6;
    entry_reduce_row(T->K[b].entry, comp, total, n_part, partial, &out[(size_t)b * 6 + comp]);
}

__global__ __launch_bounds__(RIGID_BLOCK) void rigid_integrate_kernel(const RigidTable *__restrict__ T, const long long *__restrict__ total, const double *__restrict__ rows, const double dt,
                                                                      admm_rigid::Record *__restrict__ body) {
    const int b = threadIdx.x;
    if (b >= T->n) return;
    const admm_rigid::Const K = T->K[b];
    const admm_rigid::Record S = body[b];
    const double Fe[3] = {rows[6 * b], rows[6 * b + 1], rows[6 * b + 2]}, Te[3] = {rows[6 * b + 3], rows[6 * b + 4], rows[6 * b + 5]};
    admm_rigid::Record O;
    admm_rigid::step(K, S, Fe, Te, (int64_t)total[K.entry], dt, O);
    body[b] = O;
}

__global__ __launch_bounds__(RIGID_BLOCK) void rigid_pose_kernel(const RigidTable *__restrict__ T, const admm_rigid::Record *__restrict__ body, ShapeTable *__restrict__ shapes) {
    const int b = threadIdx.x;
    if (b >= T->n) return;
    const int e = T->K[b].entry;
    if (e < 0 || e >= ADMM_MAX_SHAPES) return;
    const admm_rigid::Record S = body[b];
    double par[4], frame[12], motion[9];
    const int framed = admm_rigid::pose(S, par, frame, motion);
#pragma unroll
    for (int j = 0; j < 4; ++j) shapes->par[e][j] = par[j];
#pragma unroll
    for (int k = 0; k < 12; ++k) shapes->frame[e][k] = frame[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) shapes->motion[e][k] = motion[k];
    shapes->framed[e] = framed;
}

// one lane: a body's acceleration, from kernel arguments (admm_hip_set_rigid_accel; no host buffer has to outlive the call)
__global__ __launch_bounds__(RIGID_BLOCK) void rigid_set_accel_kernel(RigidTable *__restrict__ T, const int b, const double a0, const double a1, const double a2) {
    if (threadIdx.x == 0 && b >= 0 && b < T->n) { T->K[b].accel[0] = a0; T->K[b].accel[1] = a1; T->K[b].accel[2] = a2; }
}

} // namespace admm_dev
