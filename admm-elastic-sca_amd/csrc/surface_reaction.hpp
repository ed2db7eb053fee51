// surface_reaction.hpp -- two-way contact: the reaction of a contact handed to the nodes of the body or sheet surface it landed on;
// shared by the host (surface_reaction_host.cpp: admm_hip_surface_reaction_query) and the device (kernels_surface_reaction.hpp).  Both
// sides compile it with -ffp-contract=off and keep the operation order below, so they give the same bits.  Extension, no reference
// counterpart.
//
// Per frame, after the epilogue and before the velocity damping, on the v the epilogue left.  The contacts k = 0 .. K - 1 are the
// list of admm_hip_get_contacts(depth_min): ascending caller's node index, f_k the node's f_contact, point_k; entry_k the owner entry
// of admm_hip_get_contact_owners.  Classification (classify; the first line that holds decides):
//   UNOWNED   entry_k < 0
//   OTHER     the entry is not an ADMM_SHAPE_MESH, or its mesh M is not a surface of simulated nodes, or M's share s_M is not > 0
//   SELF      the contacting node is one of M's own nodes (the owner range of the surface; such contacts do not react here)
//   REACTING  otherwise
// The hit of a reacting contact: point_k in the entry's coordinates as the collision rule takes it there (frame, then translation),
// the unbounded admm_mesh::closest on M as this frame's start rebuilt it (ties: the lowest original triangle), lambda = tri_weights at
// the hit, the corners cid[3 orig + c], c = 0, 1, 2, mapped to nodes by the surface's vertex -> node table.
//
// Operation order.  Every product is rounded, no fused multiply-adds.
//   impulse        p_j = dt * f_j                      once per contact, j = 0, 1, 2
//   share weight   g_c = s_M * lambda_c                 per corner
//   contribution   q_cj = g_c * p_j                     per corner and component (contribution)
//   per destination node t, over its contributions in ascending (contact index k, corner c):
//                  a_j = 0.0;  a_j = a_j + q_cj         (one addition per contribution, in that order)
//                  dv_j = a_j / m_tj;   v_j = v_j - dv_j          (apply; m_tj the node's mass entry of component j)
// A node with no contribution is not touched and keeps its bits.
//
// Properties.  Linear momentum: sum_t m_t dv_t = dt sum_k s_k f_k up to rounding, because the weights of a hit add up to one.
// Friction's tangential part is inside f and reacts too.  The load is explicit: no term in the energies or the objective, and it
// lags the push by one frame.  Angular momentum is not exact: the force acts at the node, the reaction at the surface's closest
// point, a contact depth apart.
#pragma once
#include <stdint.h>
#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_surface_reaction {

enum Status { REACTING = 0, UNOWNED = 1, OTHER = 2, SELF = 3 };

// = admm_hip_surface_contact (include/admm_hip.h)
struct Record { int32_t node, mesh, tri, corner[3], status, pad_; double weight[3], share; };
static_assert(sizeof(Record) == 64, "the record is 64 bytes");

// is_surface_mesh: the entry names a mesh whose vertices are simulated nodes; own: the contacting node is one of that mesh's own nodes
ADMM_HD int classify(const int entry, const bool is_surface_mesh, const double share, const bool own) {
    if (entry < 0) return UNOWNED;
    if (!is_surface_mesh || !(share > 0.0)) return OTHER;
    return own ? SELF : REACTING;
}

ADMM_HD void impulse(const double dt, const double *f, double *p) { p[0] = dt * f[0]; p[1] = dt * f[1]; p[2] = dt * f[2]; }
// one corner's contribution q[3] from the contact's impulse p[3]
ADMM_HD void contribution(const double share, const double lambda, const double *p, double *q) {
    const double g = share * lambda;
    q[0] = g * p[0]; q[1] = g * p[1]; q[2] = g * p[2];
}
ADMM_HD void accumulate(const double *q, double *a) { a[0] = a[0] + q[0]; a[1] = a[1] + q[1]; a[2] = a[2] + q[2]; }
// a[3]: the node's sum, m[3]: its mass entries -> dv[3], and v[3] updated
ADMM_HD void apply(const double *a, const double *m, double *dv, double *v) {
    for (int j = 0; j < 3; ++j) { dv[j] = a[j] / m[j]; v[j] = v[j] - dv[j]; }
}

// the number of 8-bit passes of the stable sort for keys in [0, key_bound): the digits of key_bound - 1, at least one
ADMM_HD int sort_passes(const long long key_bound) {
    int p = 1;
    for (long long top = (key_bound - 1) >> 8; top > 0; top >>= 8) ++p;
    return p;
}

} // namespace admm_surface_reaction
