// mesh_query.hpp -- triangle-mesh obstacles (ADMM_SHAPE_MESH: closed meshes, and open surfaces as thick shells): the point query shared by the host (mesh.cpp:
// admm_hip_mesh_query, the class mirror's CollisionMesh) and the device (kernels_collision.hpp project_collision_mesh_kernel).
// Both sides compile it with -ffp-contract=off and run the same traversal in the same order, so they give the same bits.
//
// Query of a point q (already relative to the instance's translation):
//   closest point c = the minimum over all triangles of (|q - c_i|^2, original triangle index), compared lexicographically --
//   ties go to the lowest index, so the result does not depend on the BVH or the traversal order; c_i from ONE closest-point
//   routine that also classifies q into the triangle's vertex / edge / face region (Ericson, Real-Time Collision Detection 5.1.5);
//   inside  iff  q lies strictly inside the root box and dot(q - c, n) < 0, n = the pseudo-normal of c's feature (face normal, sum of
//   the edge's two face normals, angle-weighted vertex normal; Baerentzen & Aanaes 2005), all precomputed on the host.
//
// Open surfaces (admm_hip_mesh_create_open: boundary edges allowed) collide as thick shells.  A shell of half thickness r > 0 occupies
// every point whose distance to the surface is below r.  The rule is unsigned -- no inside, no outside: a point is pushed to distance r
// on the side it is on.  For a candidate q (relative to the instance's translation t, in local coordinates under a frame), every
// product and sum rounded, no fused multiply-adds, in this order:
//   1. box test   the traversal runs only when  lo_j - r < q_j < hi_j + r  holds strictly for j = 0, 1, 2 (lo, hi: the root box; in_shell_box);
//                 a point that fails keeps its bits
//   2. hit        h = closest_within(q, r * r): the hit of `closest` whenever that one's d2 < r * r, slot = -1 otherwise
//   3. decision   the point collides exactly when  h.slot >= 0 && h.d2 < r * r
//   4. push       e_j = q_j - c_j,  d = sqrt(h.d2);   d > 0:  s = r / d,  p'_j = c_j + s * e_j;
//                 d == 0:  p'_j = c_j + r * n_j,  n = the unit face normal of the winning triangle (Nrm::n[0])          (shell_push)
//   5. world      p_j = t_j + p'_j, then under a frame to_world -- only for a point that was moved
// Without side memory the rule does not know on which side a node started the frame: a node that crosses the mid-surface within one
// frame leaves on the far side, so callers keep r above closing speed x dt.
//
// Side memory (admm_hip_set_collision_mesh_side_memory: an open mesh with a reach R, finite, R >= r > 0).  The context keeps one int32
// side s per node and such mesh: +1 the side the surface's normals point to, -1 the other one, 0 none.  For a hit h of q:
//   g = (q0 - c0) n0 + (q1 - c1) n1 + (q2 - c2) n2,  n = feature_normal(nrm[h.slot], h.reg)   (the expression `inside` evaluates; side_g)
//   side_of = +1 for g > 0, -1 for g < 0, else 0
//   a boundary hit: h's feature is a boundary edge (adj = -1) or a vertex incident to one -- bit h.reg (1..6) of bnd[h.slot], a table of
//   one int32 per leaf slot in the slot's rotated corner order, built once from the topology (boundary_table)
// Latch (side_latch), once per frame from the frame-start position q with the previous side s; the first step whose condition holds decides:
//   1. in_shell_box(q, root, R) fails: s' = 0        2. h = closest_within(q, R * R) finds nothing: s' = 0
//   3. h is a boundary hit: s' = 0 (a node that goes round the rim forgets)       4. s != 0: s' = s (sticky)
//   5. s == 0: s' = side_of(q, h) when h.d2 >= r * r, else 0 (never learned from inside the shell)
// Projection (sided_project), per iteration, for a node with s != 0 (s == 0: steps 1 to 5 of the shell rule above, the same code and bits):
//   1. in_shell_box(q, root, R) fails: the point keeps its bits      2. h = closest_within(q, R * R) finds nothing: it keeps its bits
//   3. a boundary hit, or side_of(q, h) * s >= 0 (or h.d2 == 0): the unsigned rule on this hit -- collides iff h.d2 < r * r, shell_push
//   4. otherwise the node has crossed: d = sqrt(h.d2) (> 0), sc = r / d, e_j = q_j - c_j, p'_j = c_j - sc * e_j: the point mirrored
//      through the closest point to distance r on the remembered side
//   5. p_j = t_j + p'_j, then under a frame to_world -- only for a point that was moved
// With memory callers keep R above closing speed x dt + r, at the cost of a traversal bounded by R instead of r.  A self-colliding sheet's
// own nodes keep the unsigned rule (their side stays 0): in the flat parts of a cloth the nearest triangle outside the 1-ring lies in the
// node's own plane, so the sign there is noise.
//
// Self-collision of a sheet (admm_hip_set_sheet_self_collision): a node that is vertex vi of the surface runs steps 1 to 5 with one change
// in step 2 -- closest_within_excluding leaves out every triangle that has vi as a corner (the node's 1-ring: cid[3 orig + k] == vi for
// k = 0, 1, 2); among the others the winner is the minimum of (d2, original triangle index) with d2 < r * r, as before.
//
// Self-collision of a closed body surface (admm_hip_set_body_self_collision: a body surface S with a half gap r > 0, a reach R >= r and a
// rest radius rho >= R).  X: the surface's vertices as admm_hip_add_body_surface registered them, the rest shape; later updates do not
// change it.  A body surface has no translation and no frame.  An interior node of the body (no vertex of S) skips S as before.  A
// surface node, vertex vi of S, with candidate q (body_self_project), every product and sum rounded, in this order:
//   1. box test   in_shell_box(q, root, R) fails: the point keeps its bits
//   2. search     closest_within_rest_excluding: the minimum of (d2, original triangle index), d2 < R * R, over the triangles that are
//                 not rest-near vi.  Triangle T with corners a, b, c = cid[3 orig + 0..2], in that order, is rest-near when
//                 closest_on_tri(X[vi], {X[a], X[b], X[c]}) gives e0 * e0 + e1 * e1 + e2 * e2 < rho * rho (rest_near; the 1-ring has
//                 e = 0).  A left-out triangle never tightens the bound; the boxes only prune (box_open), so the result does not depend
//                 on the tree.  The test is evaluated lazily, only for a triangle whose d2 would make it the new best: the winner and its
//                 bits are the definition's.  No hit: the point keeps its bits
//   3. push       g = side_g(q, h).  g >= 0 (or not a number) or d2 == 0: the unsigned rule on this hit -- collides iff d2 < r * r,
//                 shell_push.  g < 0: the node has crossed the skin and is mirrored to distance r outside: d = sqrt(d2), sc = r / d,
//                 e_j = q_j - c_j, p'_j = c_j - sc * e_j   (steps 3 and 4 of the side-memory projection with s = +1, no boundary hits)
// Everything after the push is what every mesh entry does.  Nodes of other bodies meet S by the closed-mesh rule.  Callers keep R above
// closing speed x dt + r, rho above R by the compression the body is expected to see, and rho below the body's thinnest part (or the
// two faces of a thin plate never see each other).
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

// a registered mesh as the device sees it (admm_hip_ctx::d_meshes); owner >= 0: the collision elements of nodes whose body tag equals it
// skip this mesh (admm_hip_set_collision_mesh_owner, admm_hip_add_body_surface), -1: no owner
struct MeshDev { const Node *nodes; const Tri *tris; const Nrm *nrm; int n_nodes, n_tris, owner; };
// what the moving form of the friction kernel needs of a mesh beside MeshDev (admm_hip_ctx::d_mesh_motion, parallel to d_meshes): the
// corner vertex ids of every original triangle, the vertices' velocities [nv][3] (null: none set), and for a body surface (body != 0)
// the coefficient that replaces the entry's (admm_hip_set_body_surface_friction)
struct MeshMotion { const int *cid; const double *vel; double mu; int body, pad; };

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

// the barycentric weights b[3] (corners a, b, c) of the point closest_on_tri returns for p in region reg: the expressions it evaluates,
// recomputed for one triangle (the winning one of a query: the friction kernel's vertex-velocity interpolation).  A vertex region: 1 on
// that corner; an edge: (1 - t, t) on its two corners in the order of the region's name; the face: (1 - sv - sw, sv, sw).
ADMM_HD void tri_weights(const double *p, const double *v, const int reg, double *w) {
    const double *a = v, *b = v + 3, *c = v + 6;
    w[0] = w[1] = w[2] = 0.0;
    if (reg == R_VA) { w[0] = 1.0; return; }
    if (reg == R_VB) { w[1] = 1.0; return; }
    if (reg == R_VC) { w[2] = 1.0; return; }
    const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
    const double ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const double ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
    const double d1 = ab0 * ap0 + ab1 * ap1 + ab2 * ap2, d2 = ac0 * ap0 + ac1 * ap1 + ac2 * ap2;
    const double bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
    const double d3 = ab0 * bp0 + ab1 * bp1 + ab2 * bp2, d4 = ac0 * bp0 + ac1 * bp1 + ac2 * bp2;
    if (reg == R_EAB) { const double t = d1 / (d1 - d3); w[0] = 1.0 - t; w[1] = t; return; }
    const double cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
    const double d5 = ab0 * cp0 + ab1 * cp1 + ab2 * cp2, d6 = ac0 * cp0 + ac1 * cp1 + ac2 * cp2;
    if (reg == R_ECA) { const double t = d2 / (d2 - d6); w[0] = 1.0 - t; w[2] = t; return; }
    if (reg == R_EBC) { const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6)); w[1] = 1.0 - t; w[2] = t; return; }
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double den = 1.0 / (va + vb + vc);
    const double sv = vb * den, sw = vc * den;
    w[0] = (1.0 - sv) - sw; w[1] = sv; w[2] = sw;
}
// a field given at the corners (fa, fb, fc: 3 doubles each), interpolated with the weights:  o_j = w0 fa_j + (w1 fb_j + w2 fc_j)
ADMM_HD void tri_interpolate(const double *w, const double *fa, const double *fb, const double *fc, double *o) {
    for (int j = 0; j < 3; ++j) o[j] = w[0] * fa[j] + (w[1] * fb[j] + w[2] * fc[j]);
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

// `closest` started from the bound r2: no box farther than sqrt(r2) is opened (box_open's tie margin aside), only a triangle with
// d2 < r2 is taken.  The hit of `closest` whenever that one's d2 < r2 (the winner's boxes pass box_open against any bound >= its d2, as
// they do there); otherwise slot = -1 and d2 = INFINITY.
template <class Stack>
ADMM_HD void closest_within(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const double *q, const double r2, Stack &stk, Hit &h) {
    h.d2 = r2; h.slot = -1; h.reg = 0; h.c[0] = h.c[1] = h.c[2] = 0.0;
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
                if (d2 < r2 && closer(d2, oi, h.d2, best_i)) { h.d2 = d2; best_i = oi; h.slot = t; h.reg = reg; h.c[0] = o[0]; h.c[1] = o[1]; h.c[2] = o[2]; }
            }
        } else {
            const int l = n.a, r = n.a + 1;
            const double dl = box_d2(q, nodes[l]), dr = box_d2(q, nodes[r]);
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
    if (h.slot < 0) h.d2 = INFINITY;
}

// `closest_within` without the triangles that have vertex skip_vertex as a corner (cid: the corner vertex ids [nt][3] by original
// triangle): the minimum of (d2, original triangle index) over the others, d2 < r2.  The test comes before the triangle's distance, so a
// left-out triangle never tightens the bound; the boxes only prune (box_open), so the result does not depend on the tree.
// skip_vertex < 0: nothing is left out, cid is not read, and every operation is closest_within's -- the same bits, ties included.
template <class Stack>
ADMM_HD void closest_within_excluding(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const int *__restrict__ cid, const int skip_vertex,
                                      const double *q, const double r2, Stack &stk, Hit &h) {
    h.d2 = r2; h.slot = -1; h.reg = 0; h.c[0] = h.c[1] = h.c[2] = 0.0;
    int best_i = NO_TRI;
    int sp = 0, cur = 0;
    for (;;) {
        const Node &n = nodes[cur];
        int next = -1;
        if (n.cnt > 0) {
            for (int t = n.a; t < n.a + n.cnt; ++t) {
                const int oi = tris[t].orig;
                if (skip_vertex >= 0) {
                    const int *c = cid + 3 * (size_t)oi;
                    if (c[0] == skip_vertex || c[1] == skip_vertex || c[2] == skip_vertex) continue;
                }
                double o[3]; int reg;
                closest_on_tri(q, tris[t].v, o, reg);
                const double e0 = q[0] - o[0], e1 = q[1] - o[1], e2 = q[2] - o[2];
                const double d2 = e0 * e0 + e1 * e1 + e2 * e2;
                if (d2 < r2 && closer(d2, oi, h.d2, best_i)) { h.d2 = d2; best_i = oi; h.slot = t; h.reg = reg; h.c[0] = o[0]; h.c[1] = o[1]; h.c[2] = o[2]; }
            }
        } else {
            const int l = n.a, r = n.a + 1;
            const double dl = box_d2(q, nodes[l]), dr = box_d2(q, nodes[r]);
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
    if (h.slot < 0) h.d2 = INFINITY;
}

// ---- open surfaces as thick shells (the rule at the top of this file) ------------------------------------------------------------
// step 1: q strictly inside the root box inflated by r
ADMM_HD bool in_shell_box(const double *q, const Node &n, const double r) {
    return n.lo[0] - r < q[0] && q[0] < n.hi[0] + r && n.lo[1] - r < q[1] && q[1] < n.hi[1] + r && n.lo[2] - r < q[2] && q[2] < n.hi[2] + r;
}
// step 3
ADMM_HD bool shell_collides(const Hit &h, const double r) { return h.slot >= 0 && h.d2 < r * r; }
// step 4: o = p' (relative to the instance, like q and h.c)
ADMM_HD void shell_push(const double *q, const Hit &h, const Nrm *__restrict__ nrm, const double r, double *o) {
    const double e0 = q[0] - h.c[0], e1 = q[1] - h.c[1], e2 = q[2] - h.c[2];
    const double d = sqrt(h.d2);
    if (d > 0.0) {
        const double s = r / d;
        o[0] = h.c[0] + s * e0; o[1] = h.c[1] + s * e1; o[2] = h.c[2] + s * e2;
    } else {
        const double *n = nrm[h.slot].n[0];
        o[0] = h.c[0] + r * n[0]; o[1] = h.c[1] + r * n[1]; o[2] = h.c[2] + r * n[2];
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

// ---- side memory (the rule at the top of this file) --------------------------------------------------------------------------------
// the expression `inside` evaluates, for a hit with slot >= 0
ADMM_HD double side_g(const Nrm *__restrict__ nrm, const double *q, const Hit &h) {
    const double *n = feature_normal(nrm[h.slot], h.reg);
    return (q[0] - h.c[0]) * n[0] + (q[1] - h.c[1]) * n[1] + (q[2] - h.c[2]) * n[2];
}
ADMM_HD int side_of(const Nrm *__restrict__ nrm, const double *q, const Hit &h) {
    const double g = side_g(nrm, q, h);
    return g > 0.0 ? 1 : (g < 0.0 ? -1 : 0);
}
// the hit's feature is a boundary edge or a vertex incident to one (the face region, reg 0, never is)
ADMM_HD bool boundary_hit(const int *__restrict__ bnd, const Hit &h) { return ((bnd[h.slot] >> h.reg) & 1) != 0; }
// the latch: the new side of a node at q (relative to the instance) whose previous side is s
template <class Stack>
ADMM_HD int side_latch(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const Nrm *__restrict__ nrm, const int *__restrict__ bnd, const double *q,
                       const int s, const double r, const double R, Stack &stk) {
    if (!in_shell_box(q, nodes[0], R)) return 0;
    Hit h;
    closest_within(nodes, tris, q, R * R, stk, h);
    if (h.slot < 0) return 0;
    if (boundary_hit(bnd, h)) return 0;
    if (s != 0) return s;
    return h.d2 >= r * r ? side_of(nrm, q, h) : 0;
}
// the projection of a node with side s != 0: true when q moves, o = p' then (relative to the instance, like q and h.c); h: the hit
// (slot -1: none within R, or the box test failed); crossed: step 4 ran
template <class Stack>
ADMM_HD bool sided_project(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const Nrm *__restrict__ nrm, const int *__restrict__ bnd, const double *q,
                           const int s, const double r, const double R, Stack &stk, Hit &h, double *o, bool &crossed) {
    crossed = false;
    h.slot = -1; h.d2 = INFINITY; h.reg = 0;
    if (!in_shell_box(q, nodes[0], R)) return false;
    closest_within(nodes, tris, q, R * R, stk, h);
    if (h.slot < 0) return false;
    if (boundary_hit(bnd, h) || side_of(nrm, q, h) * s >= 0 || !(h.d2 > 0.0)) {
        if (!shell_collides(h, r)) return false;
        shell_push(q, h, nrm, r, o);
        return true;
    }
    crossed = true;
    const double d = sqrt(h.d2);
    const double sc = r / d;
    const double e0 = q[0] - h.c[0], e1 = q[1] - h.c[1], e2 = q[2] - h.c[2];
    o[0] = h.c[0] - sc * e0; o[1] = h.c[1] - sc * e1; o[2] = h.c[2] - sc * e2;
    return true;
}

// ---- in-place deformation (admm_hip_mesh_set_vertices on the host, kernels_mesh.hpp on the device) --------------------------------
// The topology, the tree and the leaf order stay; the arithmetic below recomputes the per-triangle data and refits the boxes.  Only
// + - * / sqrt, comparisons and bit operations: correctly rounded on both sides, so the host and the device give the same bits.

constexpr int VOL_CHUNK = 256;     // the enclosed volume: partial sums over chunks of this many triangles (original order), then the partials in order

ADMM_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ADMM_HD void cross3(const double *a, const double *b, double *o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
ADMM_HD void normalize3(double *v) { const double l = sqrt(dot3(v, v)); if (l > 0.0) for (int j = 0; j < 3; ++j) v[j] /= l; }
ADMM_HD bool finite3(const double *v) { return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]); }
// std::min / std::max (the same operand order, so the same result for signed zeros)
ADMM_HD double min_d(double a, double b) { return b < a ? b : a; }
ADMM_HD double max_d(double a, double b) { return a < b ? b : a; }

// the unit normal of the triangle with corners v[9] (canonical order): false when its area is zero (or not a number)
ADMM_HD bool face_normal(const double *v, double *n) {
    double e1[3], e2[3];
    for (int j = 0; j < 3; ++j) { e1[j] = v[3 + j] - v[j]; e2[j] = v[6 + j] - v[j]; }
    cross3(e1, e2, n);
    if (!(dot3(n, n) > 0.0)) return false;
    normalize3(n);
    return true;
}
// the check of an update: the lowest original triangle with a non-finite corner or zero area (NO_TRI: none), the lowest non-finite
// vertex (NO_TRI: none; also catches vertices no triangle uses), 6 x the enclosed volume (blocked sum, VOL_CHUNK)
struct UpdateCheck { int bad_tri, bad_vtx; double vol6; };
static_assert(sizeof(UpdateCheck) == 16, "the device update reads back 16 bytes");
// the one refusal predicate of an update, shared by the host (mesh_refusal) and the device's frame-start body-surface update; an open
// mesh (a shell) encloses nothing: no volume condition
ADMM_HD bool update_refused(const UpdateCheck &c, const bool open) { return c.bad_tri != NO_TRI || c.bad_vtx != NO_TRI || (!open && !(c.vol6 > 0.0)); }
// a body surface's device record (kernels_mesh.hpp): frame-start updates applied / refused, the lowest bad triangle of the last refusal
// (-1: none), and the gate the commit kernels read (nonzero: this frame's update was refused, the live arrays stay)
struct BodyStatus { long long updated, refused; int last_bad_tri, gate; };
static_assert(sizeof(BodyStatus) == 24, "BodyStatus is read back as 24 bytes");

// the triangle's term of 6 x the enclosed volume
ADMM_HD double volume_term(const double *v) { double c[3]; cross3(v + 3, v + 6, c); return dot3(v, c); }

// the cosine of the angle at corner p between the edges to p1 and p2, clamped to [-1, 1] as std::max(-1, std::min(1, c)) does
ADMM_HD double corner_cos(const double *p, const double *p1, const double *p2) {
    double a[3], b[3];
    for (int j = 0; j < 3; ++j) { a[j] = p1[j] - p[j]; b[j] = p2[j] - p[j]; }
    const double c = dot3(a, b) / sqrt(dot3(a, a) * dot3(b, b));
    const double m = c < 1.0 ? c : 1.0;
    return -1.0 < m ? m : -1.0;
}

// acos on [-1, 1] from + - * / sqrt and one bit mask (the classic rational approximation of asin, Cody & Waite / fdlibm's scheme):
// within an ulp of the libm value, and the same bits on the host and the device -- the vertex pseudo-normals of a deformed mesh
ADMM_HD double acos_rt(double x) {
    const double pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    if (x >= 1.0) return 0.0;
    if (x <= -1.0) return pi + 2.0 * pio2_lo;
    const double ax = x < 0.0 ? -x : x;
    if (ax < 0.5) {
        if (ax <= 0x1p-57) return pio2_hi + pio2_lo;
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        return pio2_hi - (x - (pio2_lo - x * (p / q)));
    }
    const double z = (1.0 - ax) * 0.5;
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double s = sqrt(z), r = p / q;
    if (x < 0.0) return pi - 2.0 * (s + (r * s - pio2_lo));
    // x > 0.5: s split into a high part with its low 32 bits cleared and a correction, for accuracy near x = 1
    uint64_t bits; __builtin_memcpy(&bits, &s, sizeof bits);
    bits &= 0xffffffff00000000ull;
    double df; __builtin_memcpy(&df, &bits, sizeof df);
    const double c = (z - df * df) / (s + df);
    return 2.0 * (df + (r * s + c));
}

// the corners of original triangle t (canonical order cid[3t..3t+3)) gathered from verts [nv][3]
ADMM_HD void gather_tri(const double *verts, const int *cid, int t, double *v) {
    for (int k = 0; k < 3; ++k) { const double *p = verts + 3 * (size_t)cid[3 * (size_t)t + k]; v[3 * k] = p[0]; v[3 * k + 1] = p[1]; v[3 * k + 2] = p[2]; }
}
// original triangle t gathered into v[9]; false if a corner is not finite or its area is zero, else its unit normal in n[3]
ADMM_HD bool tri_ok(const double *verts, const int *cid, int t, double *v, double *n) {
    gather_tri(verts, cid, t, v);
    return finite3(v) && finite3(v + 3) && finite3(v + 6) && face_normal(v, n);
}
// the angle-weighted normal of vertex `vx`: the sum over its incidences inc[inc_ptr[vx], inc_ptr[vx + 1]) = 3 t + k, ascending (the
// order in which admm_hip_mesh_create sums them), of angle(t, k) * fn[t]
ADMM_HD void vertex_normal(const double *verts, const int *cid, const double *fn, const int *inc_ptr, const int *inc, int vx, double *o) {
    o[0] = o[1] = o[2] = 0.0;
    for (int i = inc_ptr[vx]; i < inc_ptr[vx + 1]; ++i) {
        const int t = inc[i] / 3, k = inc[i] - 3 * t;
        const int *c = cid + 3 * (size_t)t;
        const double ang = acos_rt(corner_cos(verts + 3 * (size_t)c[k], verts + 3 * (size_t)c[(k + 1) % 3], verts + 3 * (size_t)c[(k + 2) % 3]));
        for (int j = 0; j < 3; ++j) o[j] += ang * fn[3 * (size_t)t + j];
    }
}
// leaf-order slot s (original triangle t = tri.orig): its corners and the seven pseudo-normals, from the face normals fn [nt][3] and
// the (unnormalised) vertex normals vn [nv][3]; an edge's normal sums the lower-indexed face first; a boundary edge of an open mesh
// (adj < 0) takes its one face's normal
ADMM_HD void slot_data(const double *verts, const int *cid, const int *adj, const double *fn, const double *vn, Tri &tri, Nrm &N) {
    const int t = tri.orig;
    gather_tri(verts, cid, t, tri.v);
    for (int j = 0; j < 3; ++j) N.n[0][j] = fn[3 * (size_t)t + j];
    for (int k = 0; k < 3; ++k) {
        const int o = adj[3 * (size_t)t + k];
        if (o < 0) { for (int j = 0; j < 3; ++j) N.n[1 + k][j] = fn[3 * (size_t)t + j]; }
        else {
            const int lo = t < o ? t : o, hi = t < o ? o : t;
            for (int j = 0; j < 3; ++j) N.n[1 + k][j] = fn[3 * (size_t)lo + j] + fn[3 * (size_t)hi + j];
            normalize3(N.n[1 + k]);
        }
        for (int j = 0; j < 3; ++j) N.n[4 + k][j] = vn[3 * (size_t)cid[3 * (size_t)t + k] + j];
        normalize3(N.n[4 + k]);
    }
}
// node ni's box from its triangles (a leaf, the loop order of the builder) or from its two children's boxes (already refit)
ADMM_HD void refit_node(Node *nodes, const Tri *tris, int ni) {
    Node &n = nodes[ni];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (n.cnt > 0) {
        for (int i = n.a; i < n.a + n.cnt; ++i) for (int k = 0; k < 3; ++k) for (int j = 0; j < 3; ++j) {
            const double v = tris[i].v[3 * k + j];
            lo[j] = min_d(lo[j], v); hi[j] = max_d(hi[j], v);
        }
    } else {
        const Node &l = nodes[n.a], &r = nodes[n.a + 1];
        for (int j = 0; j < 3; ++j) { lo[j] = min_d(l.lo[j], r.lo[j]); hi[j] = max_d(l.hi[j], r.hi[j]); }
    }
    for (int j = 0; j < 3; ++j) { n.lo[j] = lo[j]; n.hi[j] = hi[j]; }
}

// ---- self-collision of a closed body surface (the rule at the top of this file) ---------------------------------------------------
// original triangle oi is rest-near vertex vi: its distance to X[vi] in the rest shape X [nv][3] is below rho (rho2 = rho * rho)
ADMM_HD bool rest_near(const double *__restrict__ rest, const int *__restrict__ cid, const int oi, const int vi, const double rho2) {
    double v[9], o[3]; int reg;
    gather_tri(rest, cid, oi, v);
    const double *p = rest + 3 * (size_t)vi;
    closest_on_tri(p, v, o, reg);
    const double e0 = p[0] - o[0], e1 = p[1] - o[1], e2 = p[2] - o[2];
    return e0 * e0 + e1 * e1 + e2 * e2 < rho2;
}
// `closest_within` over the triangles that are not rest-near vertex vi: the minimum of (d2, original triangle index), d2 < r2.  The rest
// test runs only for a triangle that would become the new best (the gathers of the rest shape stay off every other triangle); one that
// fails it is passed over and never tightens the bound, so the winner is the one an eager test before the distance gives.
template <class Stack>
ADMM_HD void closest_within_rest_excluding(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const int *__restrict__ cid, const double *__restrict__ rest,
                                           const int vi, const double rho2, const double *q, const double r2, Stack &stk, Hit &h) {
    h.d2 = r2; h.slot = -1; h.reg = 0; h.c[0] = h.c[1] = h.c[2] = 0.0;
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
                if (d2 < r2 && closer(d2, oi, h.d2, best_i) && !rest_near(rest, cid, oi, vi, rho2)) {
                    h.d2 = d2; best_i = oi; h.slot = t; h.reg = reg; h.c[0] = o[0]; h.c[1] = o[1]; h.c[2] = o[2];
                }
            }
        } else {
            const int l = n.a, r = n.a + 1;
            const double dl = box_d2(q, nodes[l]), dr = box_d2(q, nodes[r]);
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
    if (h.slot < 0) h.d2 = INFINITY;
}
// the projection of a surface node, vertex vi: true when q moves, o = p' then; h: the hit (slot -1: none within R, or the box test
// failed); crossed: the mirror push ran
template <class Stack>
ADMM_HD bool body_self_project(const Node *__restrict__ nodes, const Tri *__restrict__ tris, const Nrm *__restrict__ nrm, const int *__restrict__ cid,
                               const double *__restrict__ rest, const int vi, const double *q, const double r, const double R, const double rho, Stack &stk,
                               Hit &h, double *o, bool &crossed) {
    crossed = false;
    h.slot = -1; h.d2 = INFINITY; h.reg = 0;
    if (!in_shell_box(q, nodes[0], R)) return false;
    closest_within_rest_excluding(nodes, tris, cid, rest, vi, rho * rho, q, R * R, stk, h);
    if (h.slot < 0) return false;
    if (!(side_g(nrm, q, h) < 0.0) || !(h.d2 > 0.0)) {
        if (!shell_collides(h, r)) return false;
        shell_push(q, h, nrm, r, o);
        return true;
    }
    crossed = true;
    const double d = sqrt(h.d2);
    const double sc = r / d;
    const double e0 = q[0] - h.c[0], e1 = q[1] - h.c[1], e2 = q[2] - h.c[2];
    o[0] = h.c[0] - sc * e0; o[1] = h.c[1] - sc * e1; o[2] = h.c[2] - sc * e2;
    return true;
}

} // namespace admm_mesh
