// kernels_mesh.hpp -- admm_hip_update_collision_mesh after finalize: a registered mesh obstacle takes new vertex positions in place,
// in the arrays finalize uploaded (so captured graphs stay valid).  The arithmetic is mesh_query.hpp's, the same the host runs in
// admm_hip_mesh_set_vertices, so both give the same bits.  Two stages (launch.inc: update_mesh_device):
//   check   mesh_check_kernel: face normals into scratch (by original triangle), the lowest bad triangle / vertex (atomicMin: the same
//           answer whatever the schedule), the volume's partial sums over chunks of VOL_CHUNK triangles; mesh_volume_kernel sums the
//           partials in order.  The host reads the 16-byte UpdateCheck back and refuses the update before anything live is written.
//   commit  mesh_vertex_normal_kernel (one lane per vertex, its incidences in order), mesh_slot_kernel (one lane per leaf-order slot:
//           corners and the seven pseudo-normals), then mesh_refit_kernel once per BVH level, deepest first: leaves from their
//           triangles, internal nodes from their children.  One launch per level and no hand-off between workgroups.
// A body surface (admm_hip_add_body_surface; admm_hip_add_sheet_surface: an open one) runs the same stages at the start of every admm_hip_step (launch.inc: update_bodies),
// eagerly and without a read-back: mesh_gather_kernel stages its vertices from the frame-start x (device node ids mapped at finalize),
// mesh_volume_kernel takes the verdict on the device (update_refused, the predicate mesh_refusal uses) into the surface's BodyStatus,
// counts the frame and re-arms the check, and the commit kernels read the gate and return at once after a refusal, so that the last
// good surface stays.  The host-driven update passes no status and no gate and runs exactly as before.
#pragma once
#include <hip/hip_runtime.h>
#include "mesh_query.hpp"

namespace admm_dev {

constexpr int MESH_BLOCK = admm_mesh::VOL_CHUNK;      // one volume chunk per workgroup

__global__ __launch_bounds__(MESH_BLOCK) void mesh_check_kernel(int nt, int nv, const double *__restrict__ verts, const int *__restrict__ cid,
                                                               double *__restrict__ fn, double *__restrict__ part, admm_mesh::UpdateCheck *chk) {
    __shared__ double term[MESH_BLOCK];
    const int base = blockIdx.x * MESH_BLOCK, i = base + threadIdx.x;
    double s = 0.0;
    if (i < nt) {
        double v[9];
        if (!admm_mesh::tri_ok(verts, cid, i, v, fn + 3 * (size_t)i)) atomicMin(&chk->bad_tri, i);
        s = admm_mesh::volume_term(v);
    }
    if (i < nv && !admm_mesh::finite3(verts + 3 * (size_t)i)) atomicMin(&chk->bad_vtx, i);
    term[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0 && base < nt) {      // the chunk's partial sum in triangle order (as admm_hip_mesh_set_vertices)
        const int n = min(MESH_BLOCK, nt - base);
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += term[k];
        part[blockIdx.x] = acc;
    }
}

// a body surface's vertices from the simulated nodes: verts[k] = x[dnode[k]] (dnode: device node ids, fixed at finalize)
__global__ __launch_bounds__(MESH_BLOCK) void mesh_gather_kernel(int nv, const int *__restrict__ dnode, const double *__restrict__ x, double *__restrict__ verts) {
    const int k = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (k >= nv) return;
    const double *p = x + 3 * (size_t)dnode[k];
    verts[3 * (size_t)k] = p[0]; verts[3 * (size_t)k + 1] = p[1]; verts[3 * (size_t)k + 2] = p[2];
}

// ... and their velocities: vel[k] = v[dnode[k]], unless this frame's update was refused (gate: set by mesh_volume_kernel before)
__global__ __launch_bounds__(MESH_BLOCK) void mesh_gather_vel_kernel(int nv, const int *__restrict__ dnode, const double *__restrict__ v, double *__restrict__ vel,
                                                                     const int *__restrict__ gate) {
    const int k = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (k >= nv || *gate) return;
    const double *p = v + 3 * (size_t)dnode[k];
    vel[3 * (size_t)k] = p[0]; vel[3 * (size_t)k + 1] = p[1]; vel[3 * (size_t)k + 2] = p[2];
}

// one workgroup: the partials staged through LDS a block at a time (parallel loads), lane 0 adds them in order.  bs (body surfaces
// only): lane 0 also takes the verdict (open: a sheet surface, no volume condition), counts the frame, sets the commit kernels' gate and
// resets the check for the next frame
__global__ __launch_bounds__(MESH_BLOCK) void mesh_volume_kernel(int nchunk, const double *__restrict__ part, admm_mesh::UpdateCheck *chk,
                                                                admm_mesh::BodyStatus *bs, const int open) {
    __shared__ double buf[MESH_BLOCK];
    double acc = 0.0;
    for (int b = 0; b < nchunk; b += MESH_BLOCK) {
        const int n = min(MESH_BLOCK, nchunk - b);
        if ((int)threadIdx.x < n) buf[threadIdx.x] = part[b + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) for (int k = 0; k < n; ++k) acc += buf[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        chk->vol6 = acc;
        if (bs) {
            const admm_mesh::UpdateCheck c = *chk;
            const bool bad = admm_mesh::update_refused(c, open != 0);
            bs->gate = bad ? 1 : 0;
            if (bad) { bs->refused += 1; bs->last_bad_tri = c.bad_tri != admm_mesh::NO_TRI ? c.bad_tri : -1; }
            else bs->updated += 1;
            chk->bad_tri = admm_mesh::NO_TRI; chk->bad_vtx = admm_mesh::NO_TRI;
        }
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_vertex_normal_kernel(int nv, const double *__restrict__ verts, const int *__restrict__ cid,
                                                                       const double *__restrict__ fn, const int *__restrict__ inc_ptr,
                                                                       const int *__restrict__ inc, double *__restrict__ vn, const int *gate) {
    const int v = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (v >= nv || (gate && *gate)) return;
    double o[3];
    admm_mesh::vertex_normal(verts, cid, fn, inc_ptr, inc, v, o);
    vn[3 * (size_t)v] = o[0]; vn[3 * (size_t)v + 1] = o[1]; vn[3 * (size_t)v + 2] = o[2];
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_slot_kernel(int nt, const double *__restrict__ verts, const int *__restrict__ cid, const int *__restrict__ adj,
                                                              const double *__restrict__ fn, const double *__restrict__ vn, admm_mesh::Tri *tris,
                                                              admm_mesh::Nrm *nrm, const int *gate) {
    const int s = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (s >= nt || (gate && *gate)) return;
    admm_mesh::slot_data(verts, cid, adj, fn, vn, tris[s], nrm[s]);
}

// the nodes lvl[0, n) of one BVH level; the level below is already refit
__global__ __launch_bounds__(MESH_BLOCK) void mesh_refit_kernel(const int *__restrict__ lvl, int n, admm_mesh::Node *nodes, const admm_mesh::Tri *__restrict__ tris,
                                                               const int *gate) {
    const int i = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i < n && !(gate && *gate)) admm_mesh::refit_node(nodes, tris, lvl[i]);
}

} // namespace admm_dev
