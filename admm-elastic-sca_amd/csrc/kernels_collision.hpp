// kernels_collision.hpp -- the local step of CollisionForce (CollisionForce.cpp:38-70) and the latch of side memory; a part of
// kernels_local.hpp, which includes it inside namespace admm_dev after BatchDev.
//
// One element per node, D = I, one lane per element: the point p = Dx + u is pushed out of every entry of the shape list that it
// penetrates, in list order (CollisionFloor.hpp:51-58, CollisionSphere.hpp:50-66, CollisionCylinder.hpp:48-66), then u += Dx - p, z = p
// and the element's share of the right-hand side.  The list's composition selects one of eight forms, the context's attribution switch
// a ninth (launch.inc collision_form); each form knows everything the forms below it know and gives their bits on their lists (tests/test_collision_form_ladder.py holds every
// form to the bits of every form below it, on lists that a far trigger entry moves up).  A form is a kernel of its own, not a flag inside
// one: a list launches exactly the kernel of its form, and the lower forms keep their smaller register footprint.
//
//   0  project_collision_block (a segment of project_multi_kernel, or project_collision_kernel): analytic shapes only, through
//      collide_analytic (floor, sphere, z-cylinder: frame.hpp collide_round).  project_collision_mesh_kernel: with closed triangle meshes
//      in the list (ADMM_SHAPE_MESH, mesh_query.hpp), a mesh instance through a BVH traversal whose stack is the lane's column of an LDS
//      array (LdsStack: no private array indexed at run time).  A point on or outside the instance's root box cannot be inside the mesh
//      and skips the traversal.  tag (contexts with a mesh owner only, else null): the body tag of every node in device order; a node
//      skips every mesh its body owns (its own surface).
//   1  project_collision_friction_kernel<MESH>: Coulomb friction at the contacts (friction.hpp; any coefficient > 0; MESH: the context
//      has meshes registered).  After every analytic entry, and after every mesh that moved the point, admm_friction::apply clamps the
//      tangential part of p' - x0 against mu * depth (an entry that did not move the point: depth 0, nothing happens), and the next entry
//      starts from the result.  xs: the frame-start x in device order (ctx->d_x, which no kernel writes during the ADMM loop): one more
//      24-byte gather per node.
//   2  project_collision_friction_moving_kernel<MESH>: obstacles that move (collision_plan.hpp: trigger 2).  After an entry moved the
//      point and for mu > 0, w = the displacement of its surface over the frame at the contact p' (friction.hpp rigid_displacement from
//      the entry's nine doubles of shapes->motion, uniform across the wave; at a mesh hit whose mesh has vertex velocities plus dt times
//      their interpolation with the hit triangle's barycentric weights: three cid ints and three 24-byte gathers) goes into
//      admm_friction::apply_moving; a zero motion gives w = 0 and the bits of the rule at rest.  A body surface's entry takes the
//      surface's coefficient (MeshMotion::mu) in place of the entry's, which is 0 for it.  mm: null without meshes.
//   3  project_collision_framed_kernel<MESH>: a rigid frame per entry and the oriented box (frame.hpp; collision_plan.hpp: trigger 3).  For an
//      entry whose frame is not the identity (shapes->framed, uniform across the wave) the candidate goes to local coordinates, the
//      entry's unframed code runs there -- collide_round or collide_box, or for a mesh the box test, closest and inside with the
//      translation t -- and only a point that code moved goes back to world coordinates; every other point keeps its bits.  Friction
//      runs on the world-space before, p', x0 and w as in form 2; a framed mesh's interpolated vertex velocity is in the mesh's own
//      coordinates and is rotated by R first.
//   4  project_collision_shell_kernel: open meshes as thick shells (mesh_query.hpp; collision_plan.hpp: trigger 4, which implies meshes).  For an
//      entry whose mesh is open (thick[mesh] > 0, uniform across the wave) the mesh branch differs in three places: the box test is the
//      inflated one, the decision is d2 < r^2 on the hit of the search bounded by r^2, and the push target is at distance r from the
//      closest point on the side the point is on.  thick: the half thickness of every mesh, parallel to meshes (0: closed).
//   5  project_collision_self_kernel: a sheet surface that collides with itself (admm_hip_set_sheet_self_collision; collision_plan.hpp: trigger 5).
//      For an entry whose mesh the node's body owns: self[mesh] == 0 (uniform across the wave): skipped, as below; != 0: the shell branch
//      without the triangles around the node's vertex vid[node] (their corner ids: three loads per leaf triangle, per lane).  The surface
//      is the frame-start one: a node meets where the rest of the cloth was at the start of the frame.  self: the flag of every mesh,
//      parallel to meshes; vid: one id per node in device order (-1: none); both uploaded at finalize, not null in this form.
//   6  project_collision_sided_kernel: an open mesh with side memory (admm_hip_set_collision_mesh_side_memory; collision_plan.hpp sided).
//      For an entry whose mesh has a reach (reach[mesh] > 0, uniform across the wave) a lane reads its node's side
//      s = side[side_slot[mesh] * side_stride + node]: s == 0 runs the shell branch, s != 0 runs sided_project with the mesh's boundary
//      table bnd[mesh] -- the search bounded by R, the unsigned rule on the node's own side or at a boundary hit, the mirror push for a
//      node that has crossed.  A node of the body that owns the mesh holds s == 0 (the latch skips it).  self, vid: null where no sheet
//      self-collides; reach, side_slot, bnd, side: uploaded at finalize, not null in this form.
//   7  project_collision_bodyself_kernel: a closed body surface that collides with itself (admm_hip_set_body_self_collision;
//      collision_plan.hpp: trigger 7).  An entry that names a mesh the node's body owns and whose lengths bself[3 mesh ..] = {r, R, rho} have r > 0
//      (uniform per entry and body): a surface node (vid >= 0) runs body_self_project against the rest vertices rest[mesh] -- the search
//      bounded by R that passes over what is near the node in the rest shape, the unsigned rule outside, the mirror push for a node that
//      has crossed the skin (no translation, no frame: refused on a body surface) --, an interior node skips the entry.  reach,
//      side_slot, bnd, side: null where no mesh has memory.
//   8  project_collision_attributed_kernel<MESH>: contact attribution (admm_hip_enable_contact_attribution; collision_plan.hpp: the context's
//      switch, whatever the list holds).  Everything form 7 does, and per element the last entry that moved the candidate -- the bits of
//      the point behind the entry's rule and before friction differ from `before` -- with the unit direction of that push (attribution.hpp),
//      stored beside u and z in every local step, owner -1 with a zero normal included.  Entries that `continue` record nothing.  z, u
//      and the slot keep the bits of the form the list would otherwise select.  It runs in contexts without the features of forms 4 to 7:
//      which table may be null is listed at project_collision_form.
//
// In every form the loads of an element (idx, dst, w2h2, x, x0, u) are issued together at the top, and every load of an entry before
// its rule: behind the u / z stores a load would wait for them.  Forms 0 to 2 are short kernels of their own built from the pieces
// below (they push through collide_analytic, and form 1 applies the rule at rest to every analytic entry without a mu > 0 early-out);
// forms 3 to 8 are strictly nested and are instantiations of one body, project_collision_form<FORM, MESH>.  Resources and timings of
// this layout beside the one with a written-out kernel per form: profiles/collision_forms/.

// the device tables of a collision launch, filled once on the host (launch.inc collision_tables); null means what the forms above say
struct CollisionTables {
    const double *xs;                        // the frame-start x, device order
    const ShapeTable *shapes;
    const admm_mesh::MeshDev *meshes;
    const admm_mesh::MeshMotion *mm;
    const double *thick;
    const int *tag;
    const int *self, *vid;
    const double *reach; const int *side_slot; const int *const *bnd; int *side; int side_stride;      // side_stride = n_nodes
    const double *bself; const double *const *rest;
    double dt;
    // form 8 only (launch.inc launch_collision_mesh fills them per batch; null in every other launch): the batch's slice of the contact
    // attribution record, one owner per element and its normal, SoA [3][at_stride]
    int *owner; double *normal; long long at_stride;
};

// the traversal stack of mesh_query.hpp's searches: the lane's column of an LDS array int[MAX_DEPTH][LOCAL_BLOCK]
struct LdsStack { int *col; __device__ int &operator[](int i) { return col[i * LOCAL_BLOCK]; } };

struct CollisionElem { int id, ds; double s; double dx[3], u[3], p[3], x0[3]; };

// the element's loads and the candidate p = Dx + u; X0: with the node's frame-start position (the forms with friction)
template <bool X0>
__device__ __forceinline__ void collision_load(const BatchDev &b, const double *__restrict__ x, const double *__restrict__ xs, const int e, CollisionElem &c) {
    const int n = b.n;
    c.id = b.idx[e];
    c.ds = b.dst[e];      // (with the other loads: behind the u / z stores it would wait for them)
    c.s = b.w2h2[e];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c.dx[j] = 0.0 + 1.0 * x[3 * (size_t)c.id + j];
        if (b.dx_override) c.dx[j] = b.dx_override[(size_t)j * n + e];
        if constexpr (X0) c.x0[j] = xs[3 * (size_t)c.id + j];
        c.u[j] = b.u[(size_t)j * n + e];
        c.p[j] = c.dx[j] + c.u[j];
    }
}
__device__ __forceinline__ void collision_store(const BatchDev &b, const int e, const CollisionElem &c) {
    const int n = b.n;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double un = c.u[j] + (c.dx[j] - c.p[j]);
        b.u[(size_t)j * n + e] = un; b.z[(size_t)j * n + e] = c.p[j];
        b.fslot[3 * (size_t)c.ds + j] = c.s * (c.p[j] - un);
    }
}

// one analytic shape of the list pushes p out.  A list with a box or a framed entry never comes here (collision_plan.hpp: trigger 3).
__device__ __forceinline__ void collide_analytic(const ShapeTable *__restrict__ shapes, const int q, double p[3]) {
    const double c0 = shapes->par[q][0], c1 = shapes->par[q][1], c2 = shapes->par[q][2], R = shapes->par[q][3];
    admm_frame::collide_round(shapes->type[q], c0, c1, c2, R, p);
}

// The mesh branches.  qq: the candidate in the mesh's coordinates (the entry's frame and translation t taken off); -> whether the
// point collides, then h is the hit and the target is written.
// a closed mesh in forms 0 to 2: l = t + the closest point of a point strictly inside.  (project_collision_form writes these four lines
// and the shell rule out, with `continue` for the early-outs: behind a helper that returns the verdict the compiler carries the hit
// through the loop over the entries, and forms 4 and 5 go from 126 to 138 VGPRs, four waves per SIMD to three.)
__device__ __forceinline__ bool closed_mesh_push(const admm_mesh::MeshDev &m, const double *t, const double *qq, LdsStack &stk, admm_mesh::Hit &h, double *l) {
    if (!admm_mesh::in_box(qq, m.nodes[0])) return false;
    admm_mesh::closest(m.nodes, m.tris, qq, stk, h);
    if (!(admm_mesh::inside(m.nodes[0], m.nrm, qq, h) && h.d2 > 0.0)) return false;
    l[0] = t[0] + h.c[0]; l[1] = t[1] + h.c[1]; l[2] = t[2] + h.c[2];
    return true;
}
// the side that node id remembers on open mesh mi (form 6 and up); 0: the mesh has no memory or the node's body owns it (the unsigned rule)
template <int FORM>
__device__ __forceinline__ int remembered_side(const CollisionTables &T, const int mi, const int id, const bool mine, double &R) {
    if constexpr (FORM == 6) R = T.reach[mi]; else R = T.reach ? T.reach[mi] : 0.0;
    return (R > 0.0 && !mine) ? T.side[(size_t)T.side_slot[mi] * (size_t)T.side_stride + id] : 0;
}
// a body's own surface node with vertex id vi against its surface (form 7): mesh_query.hpp, self-collision of a closed body surface
__device__ __forceinline__ bool body_self_push(const admm_mesh::MeshDev &m, const int *__restrict__ cid, const double *__restrict__ rest, const int vi, const double *qq,
                                               const double *__restrict__ len, LdsStack &stk, admm_mesh::Hit &h, double *l) {
    bool crossed;
    return admm_mesh::body_self_project(m.nodes, m.tris, m.nrm, cid, rest, vi, qq, len[0], len[1], len[2], stk, h, l, crossed);
}

// after a mesh moved the point (form 2 and up): a body surface's coefficient replaces the entry's; -> whether the mesh has vertex
// velocities and mu > 0, then vi = their interpolation at the hit, turned to world axes under a frame
__device__ __forceinline__ bool mesh_contact_velocity(const admm_mesh::MeshDev &m, const admm_mesh::MeshMotion mo, const double *qq, const admm_mesh::Hit &h,
                                                      const double *f, const bool framed, double &mu, double *vi) {
    if (mo.body) mu = mo.mu;
    if (!(mo.vel && mu > 0.0)) return false;
    const admm_mesh::Tri &tr = m.tris[h.slot];
    const int *c = mo.cid + 3 * (size_t)tr.orig;
    const double *va = mo.vel + 3 * (size_t)c[0], *vb = mo.vel + 3 * (size_t)c[1], *vc = mo.vel + 3 * (size_t)c[2];
    const double a0 = va[0], a1 = va[1], a2 = va[2], b0 = vb[0], b1 = vb[1], b2 = vb[2], c0 = vc[0], c1 = vc[1], c2 = vc[2];
    double bw[3];
    admm_mesh::tri_weights(qq, tr.v, h.reg, bw);
    vi[0] = bw[0] * a0 + (bw[1] * b0 + bw[2] * c0); vi[1] = bw[0] * a1 + (bw[1] * b1 + bw[2] * c1); vi[2] = bw[0] * a2 + (bw[1] * b2 + bw[2] * c2);
    if (framed) admm_frame::rotate(f, vi, vi);
    return true;
}
// the friction rule against a surface that moves, on the world-space points (form 2 and up); vhit: with the mesh's vertex velocity vi
__device__ __forceinline__ void friction_moving(const double *motion, const double dt, const double *before, double *p, const double *x0, const bool vhit, const double *vi,
                                                const double mu) {
    if (!(mu > 0.0)) return;
    double w[3];
    admm_friction::rigid_displacement(motion, dt, p, w);
    if (vhit) { w[0] = w[0] + dt * vi[0]; w[1] = w[1] + dt * vi[1]; w[2] = w[2] + dt * vi[2]; }
    admm_friction::apply_moving(before, p, x0, w, mu);      // (a shape that did not move the point: depth 0, nothing happens)
}

// ---- form 0 -----------------------------------------------------------------------------------------------------------------------
// (a segment body of project_multi_kernel, whose code must not move: written out, the operations of collision_load<false> and
// collision_store)
__device__ __forceinline__ void project_collision_block(const BatchDev &b, const double *__restrict__ x, const ShapeTable *__restrict__ shapes, const int lb) {
    const int e = b.e0 + lb * LOCAL_BLOCK + threadIdx.x;
    const int n = b.n;
    if (e >= b.e1) return;
    const int id = b.idx[e];
    const int ds = b.dst[e];      // (with the other loads: behind the u / z stores it would wait for them)
    const double s = b.w2h2[e];
    double dx[3], u[3], p[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        dx[j] = 0.0 + 1.0 * x[3 * (size_t)id + j];
        if (b.dx_override) dx[j] = b.dx_override[(size_t)j * n + e];
        u[j] = b.u[(size_t)j * n + e];
        p[j] = dx[j] + u[j];
    }
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) collide_analytic(shapes, q, p);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double un = u[j] + (dx[j] - p[j]);
        b.u[(size_t)j * n + e] = un; b.z[(size_t)j * n + e] = p[j];
        b.fslot[3 * (size_t)ds + j] = s * (p[j] - un);
    }
}

__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_mesh_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    const int e = b.e0 + (int)blockIdx.x * LOCAL_BLOCK + threadIdx.x;
    if (e >= b.e1) return;
    CollisionElem c;
    collision_load<false>(b, x, nullptr, e, c);
    LdsStack stk{&stack[0][threadIdx.x]};
    const ShapeTable *__restrict__ shapes = T.shapes;
    const int own = T.tag ? T.tag[c.id] : -1;
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) {
        if (shapes->type[q] != ADMM_SHAPE_MESH) { collide_analytic(shapes, q, c.p); continue; }
        const admm_mesh::MeshDev m = T.meshes[(int)shapes->par[q][3]];
        if (own >= 0 && m.owner == own) continue;
        const double t[3] = {shapes->par[q][0], shapes->par[q][1], shapes->par[q][2]};
        const double qq[3] = {c.p[0] - t[0], c.p[1] - t[1], c.p[2] - t[2]};
        admm_mesh::Hit h;
        closed_mesh_push(m, t, qq, stk, h, c.p);
    }
    collision_store(b, e, c);
}

// ---- forms 1 and 2 ----------------------------------------------------------------------------------------------------------------
template <bool MESH>
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_friction_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[MESH ? admm_mesh::MAX_DEPTH : 1][LOCAL_BLOCK];
    const int e = b.e0 + (int)blockIdx.x * LOCAL_BLOCK + threadIdx.x;
    if (e >= b.e1) return;
    CollisionElem c;
    collision_load<true>(b, x, T.xs, e, c);
    LdsStack stk{&stack[0][threadIdx.x]};
    const ShapeTable *__restrict__ shapes = T.shapes;
    const int own = (MESH && T.tag) ? T.tag[c.id] : -1;
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) {
        const double before[3] = {c.p[0], c.p[1], c.p[2]};
        if (!MESH || shapes->type[q] != ADMM_SHAPE_MESH) collide_analytic(shapes, q, c.p);
        else {
            const admm_mesh::MeshDev m = T.meshes[(int)shapes->par[q][3]];
            if (own >= 0 && m.owner == own) continue;
            const double t[3] = {shapes->par[q][0], shapes->par[q][1], shapes->par[q][2]};
            const double qq[3] = {c.p[0] - t[0], c.p[1] - t[1], c.p[2] - t[2]};
            admm_mesh::Hit h;
            if (!closed_mesh_push(m, t, qq, stk, h, c.p)) continue;
        }
        admm_friction::apply(before, c.p, c.x0, shapes->mu[q]);      // (a shape that did not move the point: depth 0, nothing happens)
    }
    collision_store(b, e, c);
}

template <bool MESH>
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_friction_moving_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[MESH ? admm_mesh::MAX_DEPTH : 1][LOCAL_BLOCK];
    const int e = b.e0 + (int)blockIdx.x * LOCAL_BLOCK + threadIdx.x;
    if (e >= b.e1) return;
    CollisionElem c;
    collision_load<true>(b, x, T.xs, e, c);
    LdsStack stk{&stack[0][threadIdx.x]};
    const ShapeTable *__restrict__ shapes = T.shapes;
    const int own = (MESH && T.tag) ? T.tag[c.id] : -1;
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) {
        const double before[3] = {c.p[0], c.p[1], c.p[2]};
        double mu = shapes->mu[q];
        double vi[3] = {0.0, 0.0, 0.0};      // the mesh's vertex velocities at the hit
        bool vhit = false;
        if (!MESH || shapes->type[q] != ADMM_SHAPE_MESH) collide_analytic(shapes, q, c.p);
        else {
            const int mi = (int)shapes->par[q][3];
            const admm_mesh::MeshDev m = T.meshes[mi];
            if (own >= 0 && m.owner == own) continue;
            const double t[3] = {shapes->par[q][0], shapes->par[q][1], shapes->par[q][2]};
            const double qq[3] = {c.p[0] - t[0], c.p[1] - t[1], c.p[2] - t[2]};
            admm_mesh::Hit h;
            if (!closed_mesh_push(m, t, qq, stk, h, c.p)) continue;
            vhit = mesh_contact_velocity(m, T.mm[mi], qq, h, nullptr, false, mu, vi);
        }
        friction_moving(shapes->motion[q], T.dt, before, c.p, c.x0, vhit, vi, mu);
    }
    collision_store(b, e, c);
}

// ---- forms 3 to 8 -----------------------------------------------------------------------------------------------------------------
// what a form adds to the one below it stands under if constexpr (FORM >= ...); the tests of a table for null and of what is uniform
// across the wave are run-time tests
//
// Form 8 (contact attribution) is launched on lists of EVERY lower form, in contexts that lack the features of forms 4 to 7, so it meets
// device tables that are null.  Per table read under FORM >= 4, in form 8:
//   thick, mm   read in the mesh branch only (MESH: the context has meshes), and upload.inc upload_meshes fills both for every context
//               with a mesh: reached only where filled
//   self        tested for null (as in forms 6 and 7)
//   vid         tested for null (as in forms 6 and 7); mm[mesh].cid is read by closest_within_excluding only for a node of a sheet that
//               collides with itself, whose vid upload_meshes filled, and cid is uploaded for every mesh
//   reach       tested for null in remembered_side (as in form 7); side_slot, side: read only behind reach[mesh] > 0, and upload_meshes
//               fills reach, side_slot, bnd and side together; bnd: read only behind a side != 0, which implies the same
//   bself       tested for null (form 7 does not: it implies a self-colliding body); rest: read only behind bself[3 mesh] > 0, and
//               upload_meshes fills bself and rest together, rest[mesh] for exactly the meshes with bself[3 mesh] > 0
template <int FORM, bool MESH>
__device__ __forceinline__ void project_collision_form(const BatchDev &b, const double *__restrict__ x, const CollisionTables &T, int *stack_col) {
    static_assert(FORM >= 3 && FORM <= 8 && (MESH || FORM == 3 || FORM == 8), "forms 4 to 7 imply meshes");
    const int e = b.e0 + (int)blockIdx.x * LOCAL_BLOCK + threadIdx.x;
    if (e >= b.e1) return;
    CollisionElem c;
    collision_load<true>(b, x, T.xs, e, c);
    LdsStack stk{stack_col};
    const ShapeTable *__restrict__ shapes = T.shapes;
    const int own = (MESH && T.tag) ? T.tag[c.id] : -1;
    int vi_own = -1;      // the node's vertex id on the self-colliding surface that owns it (-1: none)
    if constexpr (FORM == 5) vi_own = T.vid[c.id];
    if constexpr (FORM >= 6) vi_own = T.vid ? T.vid[c.id] : -1;
    int at_q = -1;                                // form 8: the last entry that moved the candidate and how far (attribution.hpp)
    double at_d[3] = {0.0, 0.0, 0.0};
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) {
        const double before[3] = {c.p[0], c.p[1], c.p[2]};
        const double *f = shapes->frame[q];
        const bool framed = shapes->framed[q] != 0;
        const int ty = shapes->type[q];
        double mu = shapes->mu[q];
        double vi[3] = {0.0, 0.0, 0.0};      // the mesh's vertex velocities at the hit, world axes
        bool vhit = false;
        if (!MESH || ty != ADMM_SHAPE_MESH) {
            if (!admm_frame::collide_entry(ty, shapes->par[q], f, framed, c.p)) continue;
        } else {
            const int mi = (int)shapes->par[q][3];
            const admm_mesh::MeshDev m = T.meshes[mi];
            const bool mine = own >= 0 && m.owner == own;
            bool bs = false;      // the node's body owns the mesh and its surface collides with itself
            if constexpr (FORM == 7) bs = mine && T.bself[3 * mi] > 0.0;
            if constexpr (FORM >= 8) bs = mine && T.bself && T.bself[3 * mi] > 0.0;
            if constexpr (FORM <= 4) { if (mine) continue; }
            else if constexpr (FORM == 5) { if (mine && !T.self[mi]) continue; }
            else { if (mine && !bs && !(T.self && T.self[mi])) continue; }
            if (bs && vi_own < 0) continue;                    // an interior node
            double l[3] = {c.p[0], c.p[1], c.p[2]};
            if (framed) admm_frame::to_local(f, c.p, l);
            const double t[3] = {shapes->par[q][0], shapes->par[q][1], shapes->par[q][2]};
            const double qq[3] = {l[0] - t[0], l[1] - t[1], l[2] - t[2]};
            double r = 0.0;
            if constexpr (FORM >= 4) r = T.thick[mi];
            admm_mesh::Hit h;
            if (bs) {
                if (!body_self_push(m, T.mm[mi].cid, T.rest[mi], vi_own, qq, T.bself + 3 * mi, stk, h, l)) continue;
            } else if (r > 0.0) {
                double R = 0.0, o[3];
                int sd = 0;
                if constexpr (FORM >= 6) sd = remembered_side<FORM>(T, mi, c.id, mine, R);
                if (sd != 0) {      // a remembered side: mesh_query.hpp, projection steps 1 to 4
                    bool crossed;
                    if (!admm_mesh::sided_project(m.nodes, m.tris, m.nrm, T.bnd[mi], qq, sd, r, R, stk, h, o, crossed)) continue;
                } else {            // the shell rule (mesh_query.hpp), steps 1 to 4
                    if (!admm_mesh::in_shell_box(qq, m.nodes[0], r)) continue;
                    // the node's own sheet: without the triangles around its vertex; any other entry: skip = -1, nothing is left out and cid
                    // is not read -- closest_within's operations, which form 4 calls as such
                    if constexpr (FORM >= 5) admm_mesh::closest_within_excluding(m.nodes, m.tris, T.mm[mi].cid, mine ? vi_own : -1, qq, r * r, stk, h);
                    else admm_mesh::closest_within(m.nodes, m.tris, qq, r * r, stk, h);
                    if (!admm_mesh::shell_collides(h, r)) continue;
                    admm_mesh::shell_push(qq, h, m.nrm, r, o);
                }
                l[0] = t[0] + o[0]; l[1] = t[1] + o[1]; l[2] = t[2] + o[2];
            } else {
                if (!admm_mesh::in_box(qq, m.nodes[0])) continue;
                admm_mesh::closest(m.nodes, m.tris, qq, stk, h);
                if (!(admm_mesh::inside(m.nodes[0], m.nrm, qq, h) && h.d2 > 0.0)) continue;
                l[0] = t[0] + h.c[0]; l[1] = t[1] + h.c[1]; l[2] = t[2] + h.c[2];
            }
            if (framed) admm_frame::to_world(f, l, c.p); else { c.p[0] = l[0]; c.p[1] = l[1]; c.p[2] = l[2]; }
            vhit = mesh_contact_velocity(m, T.mm[mi], qq, h, f, framed, mu, vi);
        }
        if constexpr (FORM >= 8) {      // the point behind the rule, before friction
            if (admm_attribution::moved(before, c.p)) { at_q = q; at_d[0] = c.p[0] - before[0]; at_d[1] = c.p[1] - before[1]; at_d[2] = c.p[2] - before[2]; }
        }
        friction_moving(shapes->motion[q], T.dt, before, c.p, c.x0, vhit, vi, mu);
    }
    collision_store(b, e, c);
    if constexpr (FORM >= 8) {          // every local step writes the record, owner -1 with a zero normal included
        double nr[3] = {0.0, 0.0, 0.0};
        if (at_q >= 0) admm_attribution::normal_of(at_d, nr);
        T.owner[e] = at_q;
        T.normal[e] = nr[0]; T.normal[(size_t)T.at_stride + e] = nr[1]; T.normal[2 * (size_t)T.at_stride + e] = nr[2];
    }
}

template <bool MESH>
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_framed_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[MESH ? admm_mesh::MAX_DEPTH : 1][LOCAL_BLOCK];
    project_collision_form<3, MESH>(b, x, T, &stack[0][threadIdx.x]);
}
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_shell_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    project_collision_form<4, true>(b, x, T, &stack[0][threadIdx.x]);
}
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_self_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    project_collision_form<5, true>(b, x, T, &stack[0][threadIdx.x]);
}
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_sided_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    project_collision_form<6, true>(b, x, T, &stack[0][threadIdx.x]);
}
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_bodyself_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    project_collision_form<7, true>(b, x, T, &stack[0][threadIdx.x]);
}

// form 8: everything form 7 knows, and the record of the last mover (attribution.hpp) beside the u / z stores
template <bool MESH>
__global__ __launch_bounds__(LOCAL_BLOCK) void project_collision_attributed_kernel(BatchDev b, const double *__restrict__ x, const CollisionTables T) {
    __shared__ int stack[MESH ? admm_mesh::MAX_DEPTH : 1][LOCAL_BLOCK];
    project_collision_form<8, MESH>(b, x, T, &stack[0][threadIdx.x]);
}

// the latch of side memory (mesh_query.hpp side_latch), once per frame from the frame-start x, eager at the start of admm_hip_step
// (launch.inc: latch_sides): one lane per node in device order, the traversal stack in the lane's LDS column.  For every entry of the
// current list that names a mesh with memory (slot >= 0; a list names such a mesh once): a node whose body owns the mesh is skipped,
// any other node's side is replaced by the latch of its position in the entry's coordinates.  x = T.xs, n_nodes = T.side_stride;
// tag: null without owners.
__global__ __launch_bounds__(LOCAL_BLOCK) void collision_side_kernel(const CollisionTables T) {
    __shared__ int stack[admm_mesh::MAX_DEPTH][LOCAL_BLOCK];
    const int id = (int)blockIdx.x * LOCAL_BLOCK + threadIdx.x;
    if (id >= T.side_stride) return;
    LdsStack stk{&stack[0][threadIdx.x]};
    const ShapeTable *__restrict__ shapes = T.shapes;
    const double p[3] = {T.xs[3 * (size_t)id], T.xs[3 * (size_t)id + 1], T.xs[3 * (size_t)id + 2]};
    const int own = T.tag ? T.tag[id] : -1;
    const int ns = shapes->n;
    for (int q = 0; q < ns; ++q) {
        if (shapes->type[q] != ADMM_SHAPE_MESH) continue;
        const int mi = (int)shapes->par[q][3];
        const int sl = T.side_slot[mi];
        if (sl < 0) continue;
        const admm_mesh::MeshDev m = T.meshes[mi];
        if (own >= 0 && m.owner == own) continue;
        const double *f = shapes->frame[q];
        double l[3] = {p[0], p[1], p[2]};
        if (shapes->framed[q] != 0) admm_frame::to_local(f, p, l);
        const double qq[3] = {l[0] - shapes->par[q][0], l[1] - shapes->par[q][1], l[2] - shapes->par[q][2]};
        int *sp = T.side + (size_t)sl * (size_t)T.side_stride + id;
        *sp = admm_mesh::side_latch(m.nodes, m.tris, m.nrm, T.bnd[mi], qq, *sp, T.thick[mi], T.reach[mi], stk);
    }
}
