// mesh_query.hpp -- closed triangle-mesh obstacles (ADMM_SHAPE_MESH): the point query shared by the host (mesh.cpp:
// admm_hip_mesh_query, the class mirror's CollisionMesh) and the device (kernels_local.hpp project_collision_mesh_kernel).
// Both sides compile it with -ffp-contract=off and run the same traversal in the same order, so they give the same bits.
//
// Query of a point q (already relative to the instance's translation):
//   closest point c = the minimum over all triangles of (|q - c_i|^2, original triangle index), compared lexicographically --
//   ties go to the lowest index, so the result does not depend on the BVH or the traversal order; c_i from ONE closest-point
//   routine that also classifies q into the triangle's vertex / edge / face region (Ericson, Real-Time Collision Detection 5.1.5);
//   inside  iff  q lies strictly inside the root box and dot(q - c, n) < 0, n = the pseudo-normal of c's feature (face normal, sum of
//   the edge's two face normals, angle-weighted vertex normal; Baerentzen & Aanaes 2005), all precomputed on the host.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_mesh {

constexpr int LEAF_TRIS = 4;       // triangles per BVH leaf, at most
constexpr int MAX_DEPTH = 32;      // levels of the BVH below the root, at most (checked when the BVH is built): the traversal stack's size
constexpr int NO_TRI = 0x7fffffff;

// one BVH node, 64 bytes: the box of its triangles; cnt > 0: a leaf of triangles [a, a + cnt) (leaf order), cnt == 0: children a, a + 1
struct __attribute__((aligned(16))) Node { double lo[3], hi[3]; int a, cnt; int pad[2]; };
// one triangle in leaf order: its corners (rotated so that the lowest vertex id comes first) and its index in the caller's list
struct __attribute__((aligned(16))) Tri { double v[9]; int orig, pad; double pad2; };
// the pseudo-normals of a triangle's features: face, edges AB / BC / CA, vertices A / B / C
struct Nrm { double n[7][3]; };
static_assert(sizeof(Node) == 64, "Node is one 64-byte record");
static_assert(sizeof(Tri) == 96, "Tri is 96 bytes");

// a registered mesh as the device sees it (admm_hip_ctx::d_meshes)
struct MeshDev { const Node *nodes; const Tri *tris; const Nrm *nrm; int n_nodes, n_tris; };

enum Region { R_FACE = 0, R_EAB = 1, R_EBC = 2, R_ECA = 3, R_VA = 4, R_VB = 5, R_VC = 6 };

// closest point of triangle (a, b, c) to p, and the region it lies in (Ericson 5.1.5)
ADMM_HD void closest_on_tri(const double *p, const double *v, double *o, int &reg) {
    const double *a = v, *b = v + 3, *c = v + 6;
    const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
    const double ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const double ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
    const double d1 = ab0 * ap0 + ab1 * ap1 + ab2 * ap2, d2 = ac0 * ap0 + ac1 * ap1 + ac2 * ap2;
    if (d1 <= 0.0 && d2 <= 0.0) { o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; reg = R_VA; return; }
    const double bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
    const double d3 = ab0 * bp0 + ab1 * bp1 + ab2 * bp2, d4 = ac0 * bp0 + ac1 * bp1 + ac2 * bp2;
    if (d3 >= 0.0 && d4 <= d3) { o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; reg = R_VB; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double t = d1 / (d1 - d3);
        o[0] = a[0] + t * ab0; o[1] = a[1] + t * ab1; o[2] = a[2] + t * ab2; reg = R_EAB; return;
    }
    const double cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
    const double d5 = ab0 * cp0 + ab1 * cp1 + ab2 * cp2, d6 = ac0 * cp0 + ac1 * cp1 + ac2 * cp2;
    if (d6 >= 0.0 && d5 <= d6) { o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; reg = R_VC; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double t = d2 / (d2 - d6);
        o[0] = a[0] + t * ac0; o[1] = a[1] + t * ac1; o[2] = a[2] + t * ac2; reg = R_ECA; return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        o[0] = b[0] + t * (c[0] - b[0]); o[1] = b[1] + t * (c[1] - b[1]); o[2] = b[2] + t * (c[2] - b[2]); reg = R_EBC; return;
    }
    const double den = 1.0 / (va + vb + vc);
    const double sv = vb * den, sw = vc * den;
    o[0] = a[0] + ab0 * sv + ac0 * sw; o[1] = a[1] + ab1 * sv + ac1 * sw; o[2] = a[2] + ab2 * sv + ac2 * sw; reg = R_FACE;
}

// (d2, i) < (best_d2, best_i), lexicographically
ADMM_HD bool closer(double d2, int i, double best_d2, int best_i) { return d2 < best_d2 || (d2 == best_d2 && i < best_i); }

ADMM_HD double box_d2(const double *q, const Node &n) {
    double s = 0.0;
    for (int j = 0; j < 3; ++j) {
        const double lo = n.lo[j] - q[j], hi = q[j] - n.hi[j];
        const double d = lo > 0.0 ? lo : (hi > 0.0 ? hi : 0.0);
        s = s + d * d;
    }
    return s;
}
ADMM_HD double centre_d2(const double *q, const Node &n) {
    double s = 0.0;
    for (int j = 0; j < 3; ++j) { const double d = q[j] - 0.5 * (n.lo[j] + n.hi[j]); s = s + d * d; }
    return s;
}
// q strictly inside the box: only then can it be strictly inside the mesh (a point on or outside the root box skips the traversal)
ADMM_HD bool in_box(const double *q, const Node &n) {
    return q[0] > n.lo[0] && q[0] < n.hi[0] && q[1] > n.lo[1] && q[1] < n.hi[1] && q[2] > n.lo[2] && q[2] < n.hi[2];
}
// a box is skipped only when its (rounded) distance exceeds the best one by more than rounding can explain, so that a triangle whose
// computed distance ties the best one -- and may have the lower index -- is always reached
ADMM_HD bool box_open(double bd2, double best_d2) { return !(bd2 > best_d2 + best_d2 * 0x1p-40); }

struct Hit { double c[3]; double d2; int slot, reg; };

// nearest-child-first depth-first traversal.  Stack: anything indexable by [0, MAX_DEPTH) -- a plain array on the host, the lane's
// slice of an LDS array on the device.  Every internal node pushes at most its far child, so the stack never holds more than the
// tree's depth (<= MAX_DEPTH, checked when the BVH is built).
template <class Stack>
ADMM_HD void closest(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const double *q, Stack &stk, Hit &h) {
    h.d2 = INFINITY; h.slot = -1; h.reg = 0; h.c[0] = h.c[1] = h.c[2] = 0.0;
    int best_i = NO_TRI;
    int sp = 0, cur = 0;
    for (;;) {
        const Node &n = nodes[cur];
        int next = -1;
        if (n.cnt > 0) {
            for (int t = n.a; t < n.a + n.cnt; ++t) {
                double o[3]; int reg;
                closest_on_tri(q, tris[t].v, o, reg);
                const double e0 = q[0] - o[0], e1 = q[1] - o[1], e2 = q[2] - o[2];
                const double d2 = e0 * e0 + e1 * e1 + e2 * e2;
                const int oi = tris[t].orig;
                if (closer(d2, oi, h.d2, best_i)) { h.d2 = d2; best_i = oi; h.slot = t; h.reg = reg; h.c[0] = o[0]; h.c[1] = o[1]; h.c[2] = o[2]; }
            }
        } else {
            const int l = n.a, r = n.a + 1;
            const double dl = box_d2(q, nodes[l]), dr = box_d2(q, nodes[r]);
            // nearer child first; equal box distances (typically both 0: q inside both boxes) go by the distance to the boxes' centres,
            // then left -- a deep point then finds a close triangle early and prunes more
            const bool rf = dr < dl || (dr == dl && centre_d2(q, nodes[r]) < centre_d2(q, nodes[l]));
            const int near = rf ? r : l, far = rf ? l : r;
            const double dn = rf ? dr : dl, df = rf ? dl : dr;
            if (box_open(df, h.d2) && sp < MAX_DEPTH) { stk[sp] = far; ++sp; }
            if (box_open(dn, h.d2)) next = near;
        }
        while (next < 0 && sp > 0) {
            --sp;
            const int cand = stk[sp];
            if (box_open(box_d2(q, nodes[cand]), h.d2)) next = cand;
        }
        if (next < 0) break;
        cur = next;
    }
}

// the pseudo-normal of the hit's feature
ADMM_HD const double *feature_normal(const Nrm &nr, int reg) {
    switch (reg) {
    case R_EAB: return nr.n[1]; case R_EBC: return nr.n[2]; case R_ECA: return nr.n[3];
    case R_VA: return nr.n[4]; case R_VB: return nr.n[5]; case R_VC: return nr.n[6];
    default: return nr.n[0];
    }
}
// q strictly inside the mesh (q relative to the instance, h its hit)
ADMM_HD bool inside(const Node &root, const Nrm *nrm, const double *q, const Hit &h) {
    if (!in_box(q, root) || h.slot < 0) return false;
    const double *n = feature_normal(nrm[h.slot], h.reg);
    const double s = (q[0] - h.c[0]) * n[0] + (q[1] - h.c[1]) * n[1] + (q[2] - h.c[2]) * n[2];
    return s < 0.0;
}

} // namespace admm_mesh
