// mesh.cpp -- triangle-mesh obstacles (closed meshes, and open surfaces as thick shells) on the host: validation, pseudo-normals and the BVH of admm_hip_mesh_create, and
// admm_hip_mesh_query, the host evaluation of the query the device runs (mesh_query.hpp), and admm_hip_friction_query, the same for
// the contact friction rule (friction.hpp) and its moving form's vertex-velocity interpolation, and admm_hip_shape_query and
// admm_hip_mesh_query_framed, the same for an entry with a rigid frame and for the box (frame.hpp).  Context-free: a context copies a mesh
// at admm_hip_add_collision_mesh (abi_setup.inc).  Built with -ffp-contract=off like the device code, so both give the same bits.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/admm_hip.h"
#include "mesh_host.hpp"
#include "friction.hpp"
#include "frame.hpp"

using namespace admm_mesh;

namespace {

int mesh_fail(char *err, int err_len, const char *fmt, ...) {
    if (err && err_len > 0) { va_list ap; va_start(ap, fmt); vsnprintf(err, (size_t)err_len, fmt, ap); va_end(ap); }
    return ADMM_ERR_ARG;
}

void cross(const double *a, const double *b, double *o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
double dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
void normalize(double *v) { const double l = std::sqrt(dot(v, v)); if (l > 0.0) for (int j = 0; j < 3; ++j) v[j] /= l; }

struct Builder {
    const std::vector<Tri> &src;              // canonical triangles, caller's order
    std::vector<double> cen;                  // [nt][3] centroids
    std::vector<int> ord;                     // triangles in leaf order
    std::vector<Node> nodes;
    int depth = 0;
    Builder(const std::vector<Tri> &s) : src(s) {}
    void box(int b, int e, Node &n) const {
        for (int j = 0; j < 3; ++j) { n.lo[j] = INFINITY; n.hi[j] = -INFINITY; }
        for (int i = b; i < e; ++i) for (int k = 0; k < 3; ++k) for (int j = 0; j < 3; ++j) {
            const double v = src[ord[i]].v[3 * k + j];
            n.lo[j] = std::min(n.lo[j], v); n.hi[j] = std::max(n.hi[j], v);
        }
    }
    // node `ni` over ord[b, e): a leaf of at most LEAF_TRIS triangles, or split at the median of the centroids along the widest axis of
    // their bounds (stable: ties in the centroid go by the original index) with its two children appended side by side
    void build(int ni, int b, int e, int level) {
        depth = std::max(depth, level);
        Node n{}; box(b, e, n);
        if (e - b <= LEAF_TRIS) { n.a = b; n.cnt = e - b; nodes[ni] = n; return; }
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = b; i < e; ++i) for (int j = 0; j < 3; ++j) { clo[j] = std::min(clo[j], cen[3 * ord[i] + j]); chi[j] = std::max(chi[j], cen[3 * ord[i] + j]); }
        int ax = 0;
        for (int j = 1; j < 3; ++j) if (chi[j] - clo[j] > chi[ax] - clo[ax]) ax = j;
        std::sort(ord.begin() + b, ord.begin() + e, [&](int p, int q) {
            const double cp = cen[3 * p + ax], cq = cen[3 * q + ax];
            return cp < cq || (cp == cq && p < q);
        });
        const int mid = b + (e - b) / 2;
        const int l = (int)nodes.size();
        nodes.push_back(Node{}); nodes.push_back(Node{});
        n.a = l; n.cnt = 0; nodes[ni] = n;
        build(l, b, mid, level + 1);
        build(l + 1, mid, e, level + 1);
    }
};

// thickness 0: a closed mesh; > 0: an open surface (boundary edges allowed, no volume condition), a shell of that half thickness
int mesh_build(int nv, const double *verts, int nt, const int32_t *tris, double thickness, admm_hip_mesh &M, char *err, int err_len) {
    const bool open = thickness > 0.0;
    if (!open && (nv < 4 || nt < 4 || !verts || !tris)) return mesh_fail(err, err_len, "a closed mesh needs at least 4 vertices and 4 triangles (have %d, %d)", nv, nt);
    if (open && (nv < 3 || nt < 1 || !verts || !tris)) return mesh_fail(err, err_len, "an open mesh needs at least 3 vertices and 1 triangle (have %d, %d)", nv, nt);
    for (int t = 0; t < nt; ++t) for (int k = 0; k < 3; ++k)
        if (tris[3 * (size_t)t + k] < 0 || tris[3 * (size_t)t + k] >= nv)
            return mesh_fail(err, err_len, "triangle %d: vertex index %d out of range [0, %d)", t, tris[3 * (size_t)t + k], nv);
    for (int i = 0; i < 3 * nv; ++i) if (!std::isfinite(verts[i])) return mesh_fail(err, err_len, "vertex %d is not finite", i / 3);
    // canonical corners: rotated so that the lowest vertex id comes first (orientation kept), so that a triangle listed with its
    // corners rotated gives the same arithmetic
    std::vector<Tri> src((size_t)nt);
    std::vector<int> cid((size_t)nt * 3);
    std::vector<double> fn((size_t)nt * 3);      // unit face normals
    for (int t = 0; t < nt; ++t) {
        const int32_t *T = tris + 3 * (size_t)t;
        const int r = (T[1] < T[0] && T[1] <= T[2]) ? 1 : (T[2] < T[0] && T[2] < T[1]) ? 2 : 0;
        Tri &tr = src[t];
        std::memset(&tr, 0, sizeof tr);
        for (int k = 0; k < 3; ++k) { cid[3 * (size_t)t + k] = T[(k + r) % 3]; for (int j = 0; j < 3; ++j) tr.v[3 * k + j] = verts[3 * (size_t)T[(k + r) % 3] + j]; }
        tr.orig = t;
        double e1[3], e2[3], n[3];
        for (int j = 0; j < 3; ++j) { e1[j] = tr.v[3 + j] - tr.v[j]; e2[j] = tr.v[6 + j] - tr.v[j]; }
        cross(e1, e2, n);
        if (!(dot(n, n) > 0.0) || T[0] == T[1] || T[1] == T[2] || T[0] == T[2])
            return mesh_fail(err, err_len, "triangle %d (%d, %d, %d) is degenerate (zero area)", t, T[0], T[1], T[2]);
        normalize(n);
        for (int j = 0; j < 3; ++j) fn[3 * (size_t)t + j] = n[j];
    }
    // edges: every undirected edge must be used by exactly two triangles, once in each direction
    struct E { int lo, hi, t, k; bool fwd; };
    std::vector<E> es((size_t)nt * 3);
    for (int t = 0; t < nt; ++t) for (int k = 0; k < 3; ++k) {
        const int a = cid[3 * (size_t)t + k], b = cid[3 * (size_t)t + (k + 1) % 3];
        es[3 * (size_t)t + k] = E{std::min(a, b), std::max(a, b), t, k, a < b};
    }
    std::sort(es.begin(), es.end(), [](const E &p, const E &q) { return p.lo != q.lo ? p.lo < q.lo : p.hi != q.hi ? p.hi < q.hi : p.t != q.t ? p.t < q.t : p.k < q.k; });
    std::vector<int> adj((size_t)nt * 3, -1);     // the triangle on the other side of edge k of triangle t
    for (size_t i = 0; i < es.size();) {
        size_t j = i;
        while (j < es.size() && es[j].lo == es[i].lo && es[j].hi == es[i].hi) ++j;
        if (open && j - i == 1) { i = j; continue; }      // a boundary edge: adj stays -1
        if (open && j - i > 2)
            return mesh_fail(err, err_len, "edge (%d, %d) is shared by %d triangles (first: triangles %d, %d, %d): the mesh is not edge-manifold", es[i].lo, es[i].hi, (int)(j - i),
                             es[i].t, es[i + 1].t, es[i + 2].t);
        if (j - i != 2)
            return mesh_fail(err, err_len, "edge (%d, %d) is shared by %d triangle%s (first: triangle %d), not 2: the mesh is %s", es[i].lo, es[i].hi, (int)(j - i),
                             j - i == 1 ? "" : "s", es[i].t, j - i == 1 ? "open" : "not edge-manifold");
        if (es[i].fwd == es[i + 1].fwd)
            return mesh_fail(err, err_len, "edge (%d, %d) is traversed in the same direction by triangles %d and %d: inconsistent orientation (a flipped triangle)",
                             es[i].lo, es[i].hi, es[i].t, es[i + 1].t);
        adj[3 * (size_t)es[i].t + es[i].k] = es[i + 1].t;
        adj[3 * (size_t)es[i + 1].t + es[i + 1].k] = es[i].t;
        i = j;
    }
    // outward normals: the enclosed volume is positive
    double vol = 0.0;
    for (int t = 0; t < nt; ++t) { double c[3]; cross(src[t].v + 3, src[t].v + 6, c); vol += dot(src[t].v, c); }
    if (!open && !(vol > 0.0)) return mesh_fail(err, err_len, "the mesh encloses a non-positive volume (%g): its triangles must be ordered counter-clockwise seen from outside", vol / 6.0);
    // pseudo-normals: angle-weighted vertex normals, summed edge normals
    std::vector<double> vn((size_t)nv * 3, 0.0);
    for (int t = 0; t < nt; ++t) for (int k = 0; k < 3; ++k) {
        const double *p = src[t].v + 3 * k, *p1 = src[t].v + 3 * ((k + 1) % 3), *p2 = src[t].v + 3 * ((k + 2) % 3);
        double a[3], b[3];
        for (int j = 0; j < 3; ++j) { a[j] = p1[j] - p[j]; b[j] = p2[j] - p[j]; }
        double c = dot(a, b) / std::sqrt(dot(a, a) * dot(b, b));
        c = std::max(-1.0, std::min(1.0, c));
        const double ang = std::acos(c);
        for (int j = 0; j < 3; ++j) vn[3 * (size_t)cid[3 * (size_t)t + k] + j] += ang * fn[3 * (size_t)t + j];
    }
    std::vector<Nrm> nrm((size_t)nt);
    for (int t = 0; t < nt; ++t) {
        Nrm &N = nrm[t];
        for (int j = 0; j < 3; ++j) N.n[0][j] = fn[3 * (size_t)t + j];
        for (int k = 0; k < 3; ++k) {
            const int o = adj[3 * (size_t)t + k];
            if (o < 0) { for (int j = 0; j < 3; ++j) N.n[1 + k][j] = fn[3 * (size_t)t + j]; }      // a boundary edge: its one face's normal
            else {
                const int lo = std::min(t, o), hi = std::max(t, o);      // (the same sum seen from both sides)
                for (int j = 0; j < 3; ++j) N.n[1 + k][j] = fn[3 * (size_t)lo + j] + fn[3 * (size_t)hi + j];
                normalize(N.n[1 + k]);
            }
            for (int j = 0; j < 3; ++j) N.n[4 + k][j] = vn[3 * (size_t)cid[3 * (size_t)t + k] + j];
            normalize(N.n[4 + k]);
        }
    }
    // BVH
    Builder B(src);
    B.cen.resize((size_t)nt * 3);
    for (int t = 0; t < nt; ++t) for (int j = 0; j < 3; ++j) B.cen[3 * (size_t)t + j] = (src[t].v[j] + src[t].v[3 + j] + src[t].v[6 + j]) / 3.0;
    B.ord.resize(nt);
    for (int t = 0; t < nt; ++t) B.ord[t] = t;
    B.nodes.reserve(2 * (size_t)(nt / LEAF_TRIS + 1));
    B.nodes.push_back(Node{});
    B.build(0, 0, nt, 0);
    if (B.depth > MAX_DEPTH) return mesh_fail(err, err_len, "BVH depth %d exceeds %d", B.depth, MAX_DEPTH);
    M.nodes = std::move(B.nodes);
    M.tris.resize(nt); M.nrm.resize(nt);
    for (int i = 0; i < nt; ++i) { M.tris[i] = src[B.ord[i]]; M.nrm[i] = nrm[B.ord[i]]; }
    M.depth = B.depth;
    M.thickness = open ? thickness : 0.0;
    // side memory's boundary table (mesh_query.hpp): topology and leaf order never change, so it is built once
    {
        std::vector<char> vb((size_t)nv, 0);
        for (int t = 0; t < nt; ++t) for (int k = 0; k < 3; ++k)
            if (adj[3 * (size_t)t + k] < 0) vb[cid[3 * (size_t)t + k]] = vb[cid[3 * (size_t)t + (k + 1) % 3]] = 1;
        M.bnd.assign((size_t)nt, 0);
        for (int i = 0; i < nt; ++i) {
            const int t = M.tris[i].orig;
            int bits = 0;
            for (int k = 0; k < 3; ++k) {
                if (adj[3 * (size_t)t + k] < 0) bits |= 1 << (R_EAB + k);
                if (vb[cid[3 * (size_t)t + k]]) bits |= 1 << (R_VA + k);
            }
            M.bnd[i] = bits;
        }
    }
    // the topology admm_hip_mesh_set_vertices recomputes the arrays from: corners, adjacency, each vertex's incidences in ascending
    // (triangle, corner) order -- the order of the vertex-normal sum above --, the nodes by depth (children follow their parent)
    M.nv = nv;
    M.cid = std::move(cid); M.adj = std::move(adj);
    M.inc_ptr.assign((size_t)nv + 1, 0);
    for (int e = 0; e < 3 * nt; ++e) M.inc_ptr[M.cid[e] + 1]++;
    for (int v = 0; v < nv; ++v) M.inc_ptr[v + 1] += M.inc_ptr[v];
    M.inc.resize((size_t)nt * 3);
    {
        std::vector<int> pos(M.inc_ptr.begin(), M.inc_ptr.end() - 1);
        for (int e = 0; e < 3 * nt; ++e) M.inc[pos[M.cid[e]]++] = e;
    }
    std::vector<int> dep(M.nodes.size(), 0);
    for (size_t i = 0; i < M.nodes.size(); ++i)
        if (M.nodes[i].cnt == 0) dep[M.nodes[i].a] = dep[M.nodes[i].a + 1] = dep[i] + 1;
    M.lvl_ptr.assign((size_t)M.depth + 2, 0);
    for (int d : dep) M.lvl_ptr[d + 1]++;
    for (int d = 0; d <= M.depth; ++d) M.lvl_ptr[d + 1] += M.lvl_ptr[d];
    M.lvl_nodes.resize(M.nodes.size());
    {
        std::vector<int> pos(M.lvl_ptr.begin(), M.lvl_ptr.end() - 1);
        for (size_t i = 0; i < M.nodes.size(); ++i) M.lvl_nodes[pos[dep[i]]++] = (int)i;
    }
    return ADMM_OK;
}

struct HostStack { int s[MAX_DEPTH]; int &operator[](int i) { return s[i]; } };

// the shell rule (mesh_query.hpp) on q, relative to the instance: true when q collides, o = p' then; *sd = r - d, -inf where the bounded
// search found nothing or did not run
bool shell_query(const admm_hip_mesh &M, const double *q, double *o, double *sd) {
    const double r = M.thickness;
    *sd = -INFINITY;
    if (!in_shell_box(q, M.nodes[0], r)) return false;
    HostStack stk; Hit h;
    closest_within(M.nodes.data(), M.tris.data(), q, r * r, stk, h);
    if (h.slot >= 0) *sd = r - std::sqrt(h.d2);
    if (!shell_collides(h, r)) return false;
    shell_push(q, h, M.nrm.data(), r, o);
    return true;
}

// ... with the triangles around vertex `skip` left out of step 2 (closest_within_excluding; skip < 0: none, the bits of shell_query);
// *tri = the winning original triangle, -1: none
bool shell_query_excluding(const admm_hip_mesh &M, const double *q, int skip, double *o, double *sd, int *tri) {
    const double r = M.thickness;
    *sd = -INFINITY; *tri = -1;
    if (!in_shell_box(q, M.nodes[0], r)) return false;
    HostStack stk; Hit h;
    closest_within_excluding(M.nodes.data(), M.tris.data(), M.cid.data(), skip, q, r * r, stk, h);
    if (h.slot >= 0) { *sd = r - std::sqrt(h.d2); *tri = M.tris[h.slot].orig; }
    if (!shell_collides(h, r)) return false;
    shell_push(q, h, M.nrm.data(), r, o);
    return true;
}

} // namespace

namespace admm_mesh {

int mesh_refusal(const admm_hip_mesh &M, const double *verts, const UpdateCheck &c, char *err, int err_len) {
    if (!update_refused(c, M.thickness > 0.0)) return ADMM_OK;
    if (c.bad_tri != NO_TRI) {
        const int *C = M.cid.data() + 3 * (size_t)c.bad_tri;
        for (int k = 0; k < 3; ++k)
            if (!finite3(verts + 3 * (size_t)C[k])) return mesh_fail(err, err_len, "triangle %d: vertex %d is not finite", c.bad_tri, C[k]);
        return mesh_fail(err, err_len, "triangle %d (%d, %d, %d) is degenerate (zero area)", c.bad_tri, C[0], C[1], C[2]);
    }
    if (c.bad_vtx != NO_TRI) return mesh_fail(err, err_len, "vertex %d is not finite", c.bad_vtx);
    return mesh_fail(err, err_len, "the mesh encloses a non-positive volume (%g): its triangles must stay counter-clockwise seen from outside", c.vol6 / 6.0);
}

// checked first, the mesh untouched until the update is accepted; the same stages and arithmetic as the device update (kernels_mesh.hpp)
int mesh_set_vertices(admm_hip_mesh &M, int nv, const double *verts, char *err, int err_len) {
    if (err && err_len > 0) err[0] = 0;
    if (nv != M.nv || !verts) return mesh_fail(err, err_len, "%d vertices given, the mesh has %d", nv, M.nv);
    const int nt = (int)M.tris.size(), nchunk = (nt + VOL_CHUNK - 1) / VOL_CHUNK;
    std::vector<double> fn((size_t)nt * 3), part((size_t)nchunk);
    int bad = NO_TRI;
#pragma omp parallel for schedule(static) reduction(min : bad)
    for (int c = 0; c < nchunk; ++c) {
        double s = 0.0;
        for (int t = c * VOL_CHUNK; t < std::min(nt, (c + 1) * VOL_CHUNK); ++t) {
            double v[9];
            if (!tri_ok(verts, M.cid.data(), t, v, &fn[3 * (size_t)t])) bad = std::min(bad, t);
            s += volume_term(v);
        }
        part[c] = s;
    }
    UpdateCheck chk{bad, NO_TRI, 0.0};
    for (int v = 0; v < nv; ++v) if (!finite3(verts + 3 * (size_t)v)) { chk.bad_vtx = v; break; }
    for (int c = 0; c < nchunk; ++c) chk.vol6 += part[c];
    if (const int rc = mesh_refusal(M, verts, chk, err, err_len)) return rc;
    std::vector<double> vn((size_t)nv * 3);
#pragma omp parallel for schedule(static)
    for (int v = 0; v < nv; ++v) vertex_normal(verts, M.cid.data(), fn.data(), M.inc_ptr.data(), M.inc.data(), v, &vn[3 * (size_t)v]);
#pragma omp parallel for schedule(static)
    for (int s = 0; s < nt; ++s) slot_data(verts, M.cid.data(), M.adj.data(), fn.data(), vn.data(), M.tris[s], M.nrm[s]);
    for (int d = M.depth; d >= 0; --d)
        for (int i = M.lvl_ptr[d]; i < M.lvl_ptr[d + 1]; ++i) refit_node(M.nodes.data(), M.tris.data(), M.lvl_nodes[i]);
    return ADMM_OK;
}

// the rest-pose condition of a sheet that collides with itself: the lowest vertex that lies nearer than the half thickness to a triangle
// it is not a corner of (the host form of the self-collision query over the sheet's own vertices) -> true, with the triangle and the
// distance; false: none
bool sheet_rest_violation(const admm_hip_mesh &M, int *vtx, int *tri, double *dist) {
    std::vector<double> verts(3 * (size_t)M.nv, 0.0);
    for (size_t s = 0; s < M.tris.size(); ++s)
        for (int k = 0; k < 3; ++k) for (int j = 0; j < 3; ++j) verts[3 * (size_t)M.cid[3 * (size_t)M.tris[s].orig + k] + j] = M.tris[s].v[3 * k + j];
    const double r = M.thickness;
    for (int v = 0; v < M.nv; ++v) {
        if (M.inc_ptr[v] == M.inc_ptr[v + 1]) continue;      // (a vertex no triangle uses)
        HostStack stk; Hit h;
        closest_within_excluding(M.nodes.data(), M.tris.data(), M.cid.data(), v, &verts[3 * (size_t)v], r * r, stk, h);
        if (shell_collides(h, r)) { *vtx = v; *tri = M.tris[h.slot].orig; *dist = std::sqrt(h.d2); return true; }
    }
    return false;
}

// the rest-pose condition of a body surface that collides with itself (admm_hip_set_body_self_collision): the lowest vertex that the rule
// (body_self_project, mesh_query.hpp) would move where the surface M stands, with rest shape `rest` [nv][3] -> true, with the winning
// triangle and the distance; false: none
bool body_rest_violation(const admm_hip_mesh &M, const double *rest, double r, double R, double rho, int *vtx, int *tri, double *dist) {
    std::vector<double> verts(3 * (size_t)M.nv, 0.0);
    for (size_t s = 0; s < M.tris.size(); ++s)
        for (int k = 0; k < 3; ++k) for (int j = 0; j < 3; ++j) verts[3 * (size_t)M.cid[3 * (size_t)M.tris[s].orig + k] + j] = M.tris[s].v[3 * k + j];
    for (int v = 0; v < M.nv; ++v) {
        if (M.inc_ptr[v] == M.inc_ptr[v + 1]) continue;
        HostStack stk; Hit h; double o[3]; bool crossed;
        if (body_self_project(M.nodes.data(), M.tris.data(), M.nrm.data(), M.cid.data(), rest, v, &verts[3 * (size_t)v], r, R, rho, stk, h, o, crossed)) {
            *vtx = v; *tri = M.tris[h.slot].orig; *dist = std::sqrt(h.d2); return true;
        }
    }
    return false;
}

} // namespace admm_mesh

extern "C" {

int admm_hip_mesh_create(admm_hip_mesh **out, int nv, const double *verts, int nt, const int32_t *tris, char *err, int err_len) {
    if (err && err_len > 0) err[0] = 0;
    if (!out) return mesh_fail(err, err_len, "out is NULL");
    *out = nullptr;
    admm_hip_mesh *M = new (std::nothrow) admm_hip_mesh();
    if (!M) return mesh_fail(err, err_len, "out of memory");
    const int rc = mesh_build(nv, verts, nt, tris, 0.0, *M, err, err_len);
    if (rc) { delete M; return rc; }
    *out = M;
    return ADMM_OK;
}

// an open surface (a closed one is accepted too and simply is a shell): every directed edge at most once, no degenerate triangle
int admm_hip_mesh_create_open(admm_hip_mesh **out, int nv, const double *verts, int nt, const int32_t *tris, double half_thickness, char *err, int err_len) {
    if (err && err_len > 0) err[0] = 0;
    if (!out) return mesh_fail(err, err_len, "out is NULL");
    *out = nullptr;
    if (!(half_thickness > 0.0 && std::isfinite(half_thickness))) return mesh_fail(err, err_len, "half thickness %g: it must be positive and finite", half_thickness);
    admm_hip_mesh *M = new (std::nothrow) admm_hip_mesh();
    if (!M) return mesh_fail(err, err_len, "out of memory");
    const int rc = mesh_build(nv, verts, nt, tris, half_thickness, *M, err, err_len);
    if (rc) { delete M; return rc; }
    *out = M;
    return ADMM_OK;
}

int admm_hip_mesh_thickness(const admm_hip_mesh *mesh, double *r) {
    if (!mesh || !r) return ADMM_ERR_ARG;
    *r = mesh->thickness;
    return ADMM_OK;
}

// the two closest-point searches of mesh_query.hpp as they are (for tests): r2 < 0: closest, else closest_within with the bound r2;
// q relative to the instance; slot: the leaf-order slot (-1: none), tri: the original triangle index
int admm_hip_mesh_closest(const admm_hip_mesh *mesh, int64_t n, const double *q, double r2, double *c, double *d2, int32_t *slot, int32_t *reg, int32_t *tri) {
    if (!mesh || n < 0 || (n && !q)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        HostStack stk; Hit h;
        if (r2 < 0.0) closest(mesh->nodes.data(), mesh->tris.data(), q + 3 * i, stk, h);
        else closest_within(mesh->nodes.data(), mesh->tris.data(), q + 3 * i, r2, stk, h);
        if (c) for (int j = 0; j < 3; ++j) c[3 * i + j] = h.c[j];
        if (d2) d2[i] = h.d2;
        if (slot) slot[i] = h.slot;
        if (reg) reg[i] = h.reg;
        if (tri) tri[i] = h.slot >= 0 ? mesh->tris[h.slot].orig : -1;
    }
    return ADMM_OK;
}

int admm_hip_mesh_set_vertices(admm_hip_mesh *mesh, int nv, const double *verts, char *err, int err_len) {
    if (!mesh) return mesh_fail(err, err_len, "mesh is NULL");
    return mesh_set_vertices(*mesh, nv, verts, err, err_len);
}

void admm_hip_mesh_destroy(admm_hip_mesh *mesh) { delete mesh; }

int admm_hip_mesh_info(const admm_hip_mesh *mesh, int *n_tris, int *n_nodes, int *depth, double *box) {
    if (!mesh) return ADMM_ERR_ARG;
    if (n_tris) *n_tris = (int)mesh->tris.size();
    if (n_nodes) *n_nodes = (int)mesh->nodes.size();
    if (depth) *depth = mesh->depth;
    if (box) for (int j = 0; j < 3; ++j) { box[j] = mesh->nodes[0].lo[j]; box[3 + j] = mesh->nodes[0].hi[j]; }
    return ADMM_OK;
}

int admm_hip_mesh_query(const admm_hip_mesh *mesh, const double t[3], int64_t n_pts, const double *pts, double *proj, double *sdist) {
    if (!mesh || !t || n_pts < 0 || (n_pts && !pts)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n_pts; ++i) {
        const double q[3] = {pts[3 * i] - t[0], pts[3 * i + 1] - t[1], pts[3 * i + 2] - t[2]};
        if (mesh->thickness > 0.0) {      // a shell: proj = the point after the rule (the input where it does not move it), sdist = r - d
            double o[3], sd;
            const bool hit = shell_query(*mesh, q, o, &sd);
            if (proj) for (int j = 0; j < 3; ++j) proj[3 * i + j] = hit ? t[j] + o[j] : pts[3 * i + j];
            if (sdist) sdist[i] = sd;
            continue;
        }
        HostStack stk; Hit h;
        closest(mesh->nodes.data(), mesh->tris.data(), q, stk, h);
        const bool in = inside(mesh->nodes[0], mesh->nrm.data(), q, h);
        if (proj) for (int j = 0; j < 3; ++j) proj[3 * i + j] = t[j] + h.c[j];
        if (sdist) { const double d = std::sqrt(h.d2); sdist[i] = in ? d : -d; }
    }
    return ADMM_OK;
}

// the host evaluation of one analytic list entry with its frame (frame.hpp collide_entry: what project_collision_framed_kernel runs, and
// for frame NULL or the identity what the unframed kernels run)
int admm_hip_shape_query(int type, const double params[4], const double *frame, int64_t n, const double *p, double *out, int32_t *moved) {
    if (!params || n < 0 || (n && !p)) return ADMM_ERR_ARG;
    if (type != ADMM_SHAPE_FLOOR && type != ADMM_SHAPE_SPHERE && type != ADMM_SHAPE_CYLINDER && type != ADMM_SHAPE_BOX) return ADMM_ERR_ARG;
    if (type == ADMM_SHAPE_BOX) for (int k = 0; k < 3; ++k) if (!(params[k] > 0.0 && std::isfinite(params[k]))) return ADMM_ERR_ARG;
    const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const double *f = frame ? frame : ident;
    int which; double by;
    if (admm_frame::check(f, &which, &by)) return ADMM_ERR_ARG;
    const bool framed = !admm_frame::identity(f);
    for (int64_t i = 0; i < n; ++i) {
        double q[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        const bool mv = admm_frame::collide_entry(type, params, f, framed, q);
        if (out) for (int j = 0; j < 3; ++j) out[3 * i + j] = q[j];
        if (moved) moved[i] = mv ? 1 : 0;
    }
    return ADMM_OK;
}

// admm_hip_mesh_query for an instance with a frame: the query runs on q = to_local(p), proj = to_world(t + c); NULL or the identity: the
// bits of admm_hip_mesh_query
int admm_hip_mesh_query_framed(const admm_hip_mesh *mesh, const double t[3], const double *frame, int64_t n_pts, const double *pts, double *proj, double *sdist) {
    if (!mesh || !t || n_pts < 0 || (n_pts && !pts)) return ADMM_ERR_ARG;
    int which; double by;
    if (frame && admm_frame::check(frame, &which, &by)) return ADMM_ERR_ARG;
    if (!frame || admm_frame::identity(frame)) return admm_hip_mesh_query(mesh, t, n_pts, pts, proj, sdist);
    for (int64_t i = 0; i < n_pts; ++i) {
        double l[3];
        admm_frame::to_local(frame, pts + 3 * i, l);
        const double q[3] = {l[0] - t[0], l[1] - t[1], l[2] - t[2]};
        if (mesh->thickness > 0.0) {
            double o[3], sd;
            const bool hit = shell_query(*mesh, q, o, &sd);
            if (proj) {
                const double c[3] = {t[0] + o[0], t[1] + o[1], t[2] + o[2]};
                if (hit) admm_frame::to_world(frame, c, proj + 3 * i); else for (int j = 0; j < 3; ++j) proj[3 * i + j] = pts[3 * i + j];
            }
            if (sdist) sdist[i] = sd;
            continue;
        }
        HostStack stk; Hit h;
        closest(mesh->nodes.data(), mesh->tris.data(), q, stk, h);
        const bool in = inside(mesh->nodes[0], mesh->nrm.data(), q, h);
        if (proj) {
            const double c[3] = {t[0] + h.c[0], t[1] + h.c[1], t[2] + h.c[2]};
            admm_frame::to_world(frame, c, proj + 3 * i);
        }
        if (sdist) { const double d = std::sqrt(h.d2); sdist[i] = in ? d : -d; }
    }
    return ADMM_OK;
}

// the shell rule with a per-point excluded vertex (self-collision of a sheet: a node that is vertex skip_vertex[i] of the surface does not
// meet the triangles around it), the host evaluation of what project_collision_self_kernel runs: admm_hip_mesh_query_framed on an open
// mesh with closest_within_excluding in step 2.  tri: the winning original triangle (-1: none nearer than r).  skip_vertex[i] = -1 (or
// skip_vertex NULL): the bits of admm_hip_mesh_query_framed.  Refused on a closed mesh and for an id outside [-1, nv).
int admm_hip_mesh_query_excluding(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *skip_vertex, const double t[3], const double *frame,
                                  double *proj, double *sdist, int32_t *tri) {
    if (!mesh || !t || n_pts < 0 || (n_pts && !pts)) return ADMM_ERR_ARG;
    if (!(mesh->thickness > 0.0)) return ADMM_ERR_ARG;
    int which; double by;
    if (frame && admm_frame::check(frame, &which, &by)) return ADMM_ERR_ARG;
    if (skip_vertex) for (int64_t i = 0; i < n_pts; ++i) if (skip_vertex[i] < -1 || skip_vertex[i] >= mesh->nv) return ADMM_ERR_ARG;
    const bool framed = frame && !admm_frame::identity(frame);
    for (int64_t i = 0; i < n_pts; ++i) {
        double l[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (framed) admm_frame::to_local(frame, pts + 3 * i, l);
        const double q[3] = {l[0] - t[0], l[1] - t[1], l[2] - t[2]};
        double o[3] = {0.0, 0.0, 0.0}, sd; int ti;
        const bool hit = shell_query_excluding(*mesh, q, skip_vertex ? skip_vertex[i] : -1, o, &sd, &ti);
        if (proj) {
            const double c[3] = {t[0] + o[0], t[1] + o[1], t[2] + o[2]};
            if (hit && framed) admm_frame::to_world(frame, c, proj + 3 * i);
            else for (int j = 0; j < 3; ++j) proj[3 * i + j] = hit ? c[j] : pts[3 * i + j];
        }
        if (sdist) sdist[i] = sd;
        if (tri) tri[i] = ti;
    }
    return ADMM_OK;
}

// admm_hip_mesh_velocity_query at the hit of that search: the winning triangle among those that do not have skip_vertex[i] as a corner and
// lie nearer than the mesh's half thickness; a point without such a triangle gets zeros and corner ids -1
int admm_hip_mesh_velocity_query_excluding(const admm_hip_mesh *mesh, int64_t n, const double *q, const int32_t *skip_vertex, const double t[3], const double *vel,
                                           double *out, double *weights, int32_t *corner_ids) {
    if (!mesh || !t || n < 0 || (n && !q) || (out && !vel)) return ADMM_ERR_ARG;
    if (!(mesh->thickness > 0.0)) return ADMM_ERR_ARG;
    if (skip_vertex) for (int64_t i = 0; i < n; ++i) if (skip_vertex[i] < -1 || skip_vertex[i] >= mesh->nv) return ADMM_ERR_ARG;
    const double r = mesh->thickness;
    for (int64_t i = 0; i < n; ++i) {
        const double qq[3] = {q[3 * i] - t[0], q[3 * i + 1] - t[1], q[3 * i + 2] - t[2]};
        HostStack stk; Hit h;
        h.slot = -1;
        if (in_shell_box(qq, mesh->nodes[0], r))
            closest_within_excluding(mesh->nodes.data(), mesh->tris.data(), mesh->cid.data(), skip_vertex ? skip_vertex[i] : -1, qq, r * r, stk, h);
        if (h.slot < 0) {
            for (int k = 0; k < 3; ++k) { if (weights) weights[3 * i + k] = 0.0; if (corner_ids) corner_ids[3 * i + k] = -1; if (out) out[3 * i + k] = 0.0; }
            continue;
        }
        const Tri &tr = mesh->tris[h.slot];
        const int *c = mesh->cid.data() + 3 * (size_t)tr.orig;
        double b[3];
        tri_weights(qq, tr.v, h.reg, b);
        if (weights) for (int k = 0; k < 3; ++k) weights[3 * i + k] = b[k];
        if (corner_ids) for (int k = 0; k < 3; ++k) corner_ids[3 * i + k] = c[k];
        if (out) tri_interpolate(b, vel + 3 * (size_t)c[0], vel + 3 * (size_t)c[1], vel + 3 * (size_t)c[2], out + 3 * i);
    }
    return ADMM_OK;
}

// side memory (mesh_query.hpp), context-free host evaluations with the device's bits.  The latch of collision_side_kernel: the new side of
// every point from its previous one (prev NULL: all 0) for an instance of an open mesh with reach R >= r, translated by t under a frame
int admm_hip_mesh_side_latch(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *prev, double reach, const double t[3], const double *frame,
                             int32_t *side_out) {
    if (!mesh || !t || n_pts < 0 || (n_pts && (!pts || !side_out))) return ADMM_ERR_ARG;
    const double r = mesh->thickness;
    if (!(r > 0.0) || !std::isfinite(reach) || !(reach >= r)) return ADMM_ERR_ARG;
    int which; double by;
    if (frame && admm_frame::check(frame, &which, &by)) return ADMM_ERR_ARG;
    if (prev) for (int64_t i = 0; i < n_pts; ++i) if (prev[i] < -1 || prev[i] > 1) return ADMM_ERR_ARG;
    const bool framed = frame && !admm_frame::identity(frame);
    for (int64_t i = 0; i < n_pts; ++i) {
        double l[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (framed) admm_frame::to_local(frame, pts + 3 * i, l);
        const double q[3] = {l[0] - t[0], l[1] - t[1], l[2] - t[2]};
        HostStack stk;
        side_out[i] = side_latch(mesh->nodes.data(), mesh->tris.data(), mesh->nrm.data(), mesh->bnd.data(), q, prev ? prev[i] : 0, r, reach, stk);
    }
    return ADMM_OK;
}

// ... and the projection of project_collision_sided_kernel for one entry: a point with side 0 runs the shell rule (the bits of
// admm_hip_mesh_query_framed), one with side +-1 sided_project.  sdist = r - d for an unsigned push, r + d for a crossed one, -inf for
// none; tri: the winning original triangle of a push (-1: none); crossed: 1 where step 4 ran
int admm_hip_mesh_query_sided(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *side, double reach, const double t[3], const double *frame,
                              double *proj, double *sdist, int32_t *tri, int32_t *crossed) {
    if (!mesh || !t || n_pts < 0 || (n_pts && !pts)) return ADMM_ERR_ARG;
    const double r = mesh->thickness;
    if (!(r > 0.0) || !std::isfinite(reach) || !(reach >= r)) return ADMM_ERR_ARG;
    int which; double by;
    if (frame && admm_frame::check(frame, &which, &by)) return ADMM_ERR_ARG;
    if (side) for (int64_t i = 0; i < n_pts; ++i) if (side[i] < -1 || side[i] > 1) return ADMM_ERR_ARG;
    const bool framed = frame && !admm_frame::identity(frame);
    for (int64_t i = 0; i < n_pts; ++i) {
        double l[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (framed) admm_frame::to_local(frame, pts + 3 * i, l);
        const double q[3] = {l[0] - t[0], l[1] - t[1], l[2] - t[2]};
        const int s = side ? side[i] : 0;
        double o[3] = {0.0, 0.0, 0.0}, sd = -INFINITY; int ti = -1; bool hit, cr = false;
        if (s == 0) {
            hit = shell_query_excluding(*mesh, q, -1, o, &sd, &ti);
            if (!hit) { sd = -INFINITY; ti = -1; }
        } else {
            HostStack stk; Hit h;
            hit = sided_project(mesh->nodes.data(), mesh->tris.data(), mesh->nrm.data(), mesh->bnd.data(), q, s, r, reach, stk, h, o, cr);
            if (hit) { const double d = std::sqrt(h.d2); sd = cr ? r + d : r - d; ti = mesh->tris[h.slot].orig; }
        }
        if (proj) {
            const double c[3] = {t[0] + o[0], t[1] + o[1], t[2] + o[2]};
            if (hit && framed) admm_frame::to_world(frame, c, proj + 3 * i);
            else for (int j = 0; j < 3; ++j) proj[3 * i + j] = hit ? c[j] : pts[3 * i + j];
        }
        if (sdist) sdist[i] = sd;
        if (tri) tri[i] = ti;
        if (crossed) crossed[i] = cr ? 1 : 0;
    }
    return ADMM_OK;
}

// self-collision of a closed body surface (mesh_query.hpp), the context-free host evaluation of what project_collision_bodyself_kernel
// runs for a node of the body that owns the surface: point i is vertex vertex_id[i] of the mesh (-1: an interior node, skipped: proj
// is the point, tri -1), rest_verts [nv][3] the rest shape.  No translation, no frame: a body surface has neither.  sdist = r - d for
// a hit on the outside (> 0: pushed; <= 0: a hit within the reach that leaves the point alone), r + d for a crossed one, -inf for no
// hit; tri: the winning original triangle of a hit (-1: none); crossed: 1 where the mirror ran
static bool self_lengths_ok(double r, double reach, double rest_radius) {
    return std::isfinite(r) && std::isfinite(reach) && std::isfinite(rest_radius) && r > 0.0 && reach >= r && rest_radius >= reach;
}
int admm_hip_mesh_query_self(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *vertex_id, const double *rest_verts, double r, double reach,
                             double rest_radius, double *proj, double *sdist, int32_t *tri, int32_t *crossed) {
    if (!mesh || n_pts < 0 || (n_pts && (!pts || !vertex_id)) || !rest_verts) return ADMM_ERR_ARG;
    if (mesh->thickness > 0.0 || !self_lengths_ok(r, reach, rest_radius)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n_pts; ++i) if (vertex_id[i] < -1 || vertex_id[i] >= mesh->nv) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n_pts; ++i) {
        const double *q = pts + 3 * i;
        double o[3] = {0.0, 0.0, 0.0}, sd = -INFINITY; int ti = -1; bool hit = false, cr = false;
        if (vertex_id[i] >= 0) {
            HostStack stk; Hit h;
            hit = body_self_project(mesh->nodes.data(), mesh->tris.data(), mesh->nrm.data(), mesh->cid.data(), rest_verts, vertex_id[i], q, r, reach, rest_radius, stk, h, o, cr);
            if (h.slot >= 0) { const double d = std::sqrt(h.d2); sd = cr ? r + d : r - d; ti = mesh->tris[h.slot].orig; }
        }
        if (proj) for (int j = 0; j < 3; ++j) proj[3 * i + j] = hit ? o[j] : q[j];
        if (sdist) sdist[i] = sd;
        if (tri) tri[i] = ti;
        if (crossed) crossed[i] = cr ? 1 : 0;
    }
    return ADMM_OK;
}

// admm_hip_mesh_velocity_query at the hit of that search (no existing call evaluates at a given triangle): the winning triangle among
// those that are not rest-near vertex_id[i] and lie within the reach; a point without one (or with id -1) gets zeros and corner ids -1
int admm_hip_mesh_velocity_query_self(const admm_hip_mesh *mesh, int64_t n, const double *q, const int32_t *vertex_id, const double *rest_verts, double reach,
                                      double rest_radius, const double *vel, double *out, double *weights, int32_t *corner_ids) {
    if (!mesh || n < 0 || (n && (!q || !vertex_id)) || !rest_verts || (out && !vel)) return ADMM_ERR_ARG;
    if (mesh->thickness > 0.0 || !self_lengths_ok(reach, reach, rest_radius)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) if (vertex_id[i] < -1 || vertex_id[i] >= mesh->nv) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const double *qq = q + 3 * i;
        HostStack stk; Hit h;
        h.slot = -1;
        if (vertex_id[i] >= 0 && in_shell_box(qq, mesh->nodes[0], reach))
            closest_within_rest_excluding(mesh->nodes.data(), mesh->tris.data(), mesh->cid.data(), rest_verts, vertex_id[i], rest_radius * rest_radius, qq, reach * reach, stk, h);
        if (h.slot < 0) {
            for (int k = 0; k < 3; ++k) { if (weights) weights[3 * i + k] = 0.0; if (corner_ids) corner_ids[3 * i + k] = -1; if (out) out[3 * i + k] = 0.0; }
            continue;
        }
        const Tri &tr = mesh->tris[h.slot];
        const int *c = mesh->cid.data() + 3 * (size_t)tr.orig;
        double b[3];
        tri_weights(qq, tr.v, h.reg, b);
        if (weights) for (int k = 0; k < 3; ++k) weights[3 * i + k] = b[k];
        if (corner_ids) for (int k = 0; k < 3; ++k) corner_ids[3 * i + k] = c[k];
        if (out) tri_interpolate(b, vel + 3 * (size_t)c[0], vel + 3 * (size_t)c[1], vel + 3 * (size_t)c[2], out + 3 * i);
    }
    return ADMM_OK;
}

// the boundary table of a mesh as built (for tests): one int32 per leaf slot, with the slot's original triangle
int admm_hip_mesh_boundary_table(const admm_hip_mesh *mesh, int32_t *bits, int32_t *orig) {
    if (!mesh) return ADMM_ERR_ARG;
    for (size_t i = 0; i < mesh->bnd.size(); ++i) { if (bits) bits[i] = mesh->bnd[i]; if (orig) orig[i] = mesh->tris[i].orig; }
    return ADMM_OK;
}

// ... and the pseudo-normal feature_normal(nrm[slot], reg) of n (slot, reg) pairs as stored (for tests: the n of side_g)
int admm_hip_mesh_feature_normal(const admm_hip_mesh *mesh, int64_t n, const int32_t *slot, const int32_t *reg, double *out) {
    if (!mesh || n < 0 || (n && (!slot || !reg || !out))) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        if (slot[i] < 0 || slot[i] >= (int)mesh->nrm.size() || reg[i] < 0 || reg[i] > 6) return ADMM_ERR_ARG;
        const double *v = feature_normal(mesh->nrm[slot[i]], reg[i]);
        for (int j = 0; j < 3; ++j) out[3 * i + j] = v[j];
    }
    return ADMM_OK;
}

// the host evaluation of the friction rule the device applies after every shape that moved a point (friction.hpp); context-free
int admm_hip_friction_query(int64_t n, const double *p, const double *p_out, const double *x0, const double *mu, double *result, int32_t *mode) {
    if (n < 0 || (n && (!p || !p_out || !x0 || !mu))) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        double po[3] = {p_out[3 * i], p_out[3 * i + 1], p_out[3 * i + 2]};
        const int m = admm_friction::apply(p + 3 * i, po, x0 + 3 * i, mu[i]);
        if (result) for (int j = 0; j < 3; ++j) result[3 * i + j] = po[j];
        if (mode) mode[i] = m;
    }
    return ADMM_OK;
}

// ... and of its moving form: w [n][3] = the displacement of the obstacle's surface over the frame at each contact
int admm_hip_friction_query_moving(int64_t n, const double *p, const double *p_out, const double *x0, const double *w, const double *mu, double *result, int32_t *mode) {
    if (n < 0 || (n && (!p || !p_out || !x0 || !w || !mu))) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        double po[3] = {p_out[3 * i], p_out[3 * i + 1], p_out[3 * i + 2]};
        const int m = admm_friction::apply_moving(p + 3 * i, po, x0 + 3 * i, w + 3 * i, mu[i]);
        if (result) for (int j = 0; j < 3; ++j) result[3 * i + j] = po[j];
        if (mode) mode[i] = m;
    }
    return ADMM_OK;
}

// the host evaluation of the vertex-velocity interpolation the moving friction kernel does at a mesh hit: the closest point's triangle,
// its barycentric weights (mesh_query.hpp tri_weights), its corners' vertex ids, and the field vel [nv][3] interpolated with them
int admm_hip_mesh_velocity_query(const admm_hip_mesh *mesh, int64_t n, const double *q, const double t[3], const double *vel, double *out, double *weights, int32_t *corner_ids) {
    if (!mesh || !t || n < 0 || (n && !q) || (out && !vel)) return ADMM_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const double qq[3] = {q[3 * i] - t[0], q[3 * i + 1] - t[1], q[3 * i + 2] - t[2]};
        HostStack stk; Hit h;
        closest(mesh->nodes.data(), mesh->tris.data(), qq, stk, h);
        if (h.slot < 0) return ADMM_ERR_ARG;
        const Tri &tr = mesh->tris[h.slot];
        const int *c = mesh->cid.data() + 3 * (size_t)tr.orig;
        double b[3];
        tri_weights(qq, tr.v, h.reg, b);
        if (weights) for (int k = 0; k < 3; ++k) weights[3 * i + k] = b[k];
        if (corner_ids) for (int k = 0; k < 3; ++k) corner_ids[3 * i + k] = c[k];
        if (out) tri_interpolate(b, vel + 3 * (size_t)c[0], vel + 3 * (size_t)c[1], vel + 3 * (size_t)c[2], out + 3 * i);
    }
    return ADMM_OK;
}

} // extern "C"
