/*
 * admm_hip.h -- C ABI of the MI355X-native ADMM elastic solver (libadmm_hip.so).
 *
 * This is the drop-in boundary for the hot path of mattoverby/admm-elastic-sca:
 * everything admm::System::initialize()/step() does between "forces and nodes
 * are known" and "m_x/m_v hold the new state" (reference
 * deps/admm-elastic-sca/src/system/System.cpp:26-75 and :98-179) runs behind
 * these entry points, on one GPU per context.  The reference itself has no
 * FFI: its plugin surface is the C++ classes admm::System / admm::Force.  The
 * host-side mirror of those classes (admm-elastic-sca_amd/host/admm/)
 * binds to exactly the functions declared here, and so does the Python
 * plumbing used by bench.py and tests/.  Plain C types only, caller-owned
 * host buffers, int error codes (0 = ok), no exceptions across the boundary.
 *
 * Every entry point cites the reference interface it replaces.
 */
#ifndef ADMM_HIP_H
#define ADMM_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "admm_kinds.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct admm_hip_ctx admm_hip_ctx;

enum admm_hip_err {
    ADMM_OK = 0,
    ADMM_ERR_ARG = 1,        /* bad argument / call order                       */
    ADMM_ERR_HIP = 2,        /* a HIP runtime call failed (no GPU, OOM, ...)    */
    ADMM_ERR_STATE = 3,      /* not finalized / already finalized               */
    ADMM_ERR_UNSUPPORTED = 4,/* input outside the accelerated path              */
    ADMM_ERR_FACTOR = 5,     /* matrix not positive definite                    */
    ADMM_ERR_COMM = 6        /* all-reduce hook failed                          */
};

/* ---- lifetime -------------------------------------------------------------
 * replaces: admm::System::System() / ~System()            (System.hpp:31)
 * device_id < 0: host-only context (assembly + factorization work, every
 * device call returns ADMM_ERR_HIP) -- used by the CPU test-suite.          */
int  admm_hip_create(admm_hip_ctx **out, int device_id);
void admm_hip_destroy(admm_hip_ctx *ctx);
const char *admm_hip_last_error(const admm_hip_ctx *ctx);
/* run on an existing hipStream_t (e.g. torch's current stream); NULL = own stream.  Waits for the work already queued on the
 * stream it leaves (the library's or the caller's); a caller's stream is never destroyed.  Results on a caller's non-blocking
 * stream are bitwise those on the library's own: no call relies on the legacy default stream for ordering. */
int  admm_hip_set_stream(admm_hip_ctx *ctx, void *hip_stream);

/* ---- settings -------------------------------------------------------------
 * replaces: System::settings.timestep_s / admm_iters      (System.hpp:36-44)
 * dt <= 0 is repaired to 0.04 like System::initialize     (System.cpp:103-107) */
int admm_hip_set_timestep(admm_hip_ctx *ctx, double dt);

/* ---- nodes ----------------------------------------------------------------
 * replaces: System::add_nodes(x, m)                       (System.cpp:78-95)
 * x, m: [3*n_nodes] xyz-interleaved like m_x / m_masses; velocities start at 0.
 * May be called several times before finalize; returns total node count in *total. */
int admm_hip_add_nodes(admm_hip_ctx *ctx, int n_nodes, const double *x, const double *m, int *total);

/* ---- forces ---------------------------------------------------------------
 * replaces: system->forces.push_back(new <Force>(...)) for n_elems elements of
 * one kind, in order                                      (System.hpp:52;
 * constructors: Force.hpp:65, TetForce.hpp:33,54,118, TriangleForce.hpp:32,
 * BendForce.hpp:31, AnchorForce.hpp:57,88).
 * idx    : [n_elems][ADMM_KIND_NODES[kind]] node ids
 * params : [n_elems][ADMM_KIND_PARAMS[kind]]  (layout in admm_kinds.h)
 * targets: ANCHOR only, [n_elems][3] control-point positions for MovingAnchor
 *          semantics, or NULL for StaticAnchor (target = x at finalize).
 * The order of add_batch calls and of elements inside a batch is the order of
 * system->forces; it defines global_idx exactly as Force::get_selector does.
 * Returns the batch id in *batch. */
int admm_hip_add_batch(admm_hip_ctx *ctx, int kind, int n_elems, const int32_t *idx,
                       const double *params, const double *targets, int *batch);

/* ---- user-defined forces ----------------------------------------------------
 * replaces: system->forces.push_back(new <user subclass of admm::Force>): the reference's extension
 * story is "subclass admm::Force, implement get_selector + project, push it into system->forces"
 * (Force.hpp:37-57; documented at samples/singletet.cpp:100-102; System.cpp:121-124 collects the
 * selector triplets and weights, System.cpp:57-58 calls project once per ADMM iteration).
 * A generic batch is a run of consecutive user forces ("elements"): element e owns the batch rows
 * [elem_row_ptr[e], elem_row_ptr[e+1]); its selector rows come as triplets (row relative to the batch,
 * col = 3*node + component like the reference's D, value), duplicates are summed; row_weight [n_rows]
 * is what get_selector pushed into `weights`.  The batch takes its place in the order of add_batch
 * calls.  The library needs  dt^2 D^T W^2 D = K (x) I3  for every element (true whenever a row touches
 * one coordinate and the x/y/z rows look alike, as for every force of the reference); anything else is
 * refused at finalize with ADMM_ERR_UNSUPPORTED.
 * Per ADMM iteration the device evaluates D_i x for the generic rows, the rows travel to the host and
 * the hook runs the user's project() there -- user code is host code --, then z - u returns to the
 * device and joins the right-hand side through the same per-node slots as every other force.
 * The hook mirrors Force::project(dt, Dx, u, z): Dx, u, z cover ALL generic rows of the context
 * (generic batches concatenated in add order: a force's offset is the `weights.size()` it saw in
 * get_selector when only user forces push weights); it must update u and z of this rank's elements
 * (admm_hip_local_elements) and leave the rest alone.  u starts at 0 and persists; z is D*m_x at the
 * start of every frame (System.cpp:43).  No HIP graph with generic batches (host code inside the iteration).   */
typedef int (*admm_hip_project_fn)(void *user, double dt, int64_t n_rows, const double *Dx, double *u, double *z);
int admm_hip_add_generic_batch(admm_hip_ctx *ctx, int n_elems, const int32_t *elem_row_ptr, int64_t n_triplets,
                               const int32_t *trip_row, const int32_t *trip_col, const double *trip_val,
                               const double *row_weight, int *batch);
int admm_hip_set_project_hook(admm_hip_ctx *ctx, admm_hip_project_fn fn, void *user);

/* replaces: system->explicit_forces.push_back(new ExplicitForce(dir))
 * (ExplicitForce.hpp:51-59, ExplicitForce.cpp:29-39): v += dt*dir on all nodes,
 * once per frame before the ADMM loop.                                       */
int admm_hip_add_gravity(admm_hip_ctx *ctx, double gx, double gy, double gz);
/* general form: replaces explicit_forces.push_back(new ExplicitForce(dir, indices)) and
 * new WindForce(tris) (ExplicitForce.hpp:51-71).  type ADMM_EXPLICIT_CONST: idx = node ids
 * (n_idx = 0: all nodes); ADMM_EXPLICIT_WIND: idx = [n_idx][3] triangle node ids, dir = wind
 * direction.  Explicit forces are applied in the order they were added.  The reference's
 * wind loop is an omp-parallel loop that reads velocities other threads are updating and
 * scatters under an omp critical, so its result depends on the thread schedule; this library
 * reproduces the loop run serially (OMP_NUM_THREADS=1): triangle i sees the increments of the
 * triangles before it, every node is incremented in triangle order (deterministic).        */
int admm_hip_add_explicit(admm_hip_ctx *ctx, int type, const double *dir, int n_idx, const int32_t *idx, int *which);
/* replaces: CollisionForce::collisionShapes (CollisionForce.hpp:39): the shape table used by
 * every ADMM_KIND_COLLISION batch, tested in order like CollisionForce::handleCollisions
 * (CollisionForce.cpp:55-70).  types [n], params [n][4] (admm_kinds.h).  May be updated between frames. */
int admm_hip_set_collision_shapes(admm_hip_ctx *ctx, int n_shapes, const int32_t *types, const double *params);

/* ---- closed triangle-mesh obstacles ------------------------------------------------------------------------------------------
 * Extension, no reference counterpart: the reference's only route to a mesh obstacle is a user-written CollisionShape, which
 * makes its CollisionForce host-projected.  A mesh is a context-free host object; a context registers it, then the shape list
 * names it as ADMM_SHAPE_MESH { tx, ty, tz, mesh_id } (any position in the list, mixed with the analytic shapes, the same mesh
 * several times with different translations; translations may change between frames like every shape parameter).
 *   admm_hip_mesh_create    verts [nv][3], tris [nt][3] (int32): closed, edge-manifold, consistently oriented with outward
 *                           normals by the right-hand rule, no degenerate triangle.  Validates that (ADMM_ERR_ARG, the offending
 *                           edge or triangle named in err[0..err_len), NUL-terminated), computes the pseudo-normals and builds the BVH.
 *   admm_hip_mesh_query     host evaluation for n_pts points [n][3] of the instance translated by t[3]: proj [n][3] = t + c with c the
 *                           closest point of the mesh to p - t (ties: lowest triangle index), sdist [n] = +|p - t - c| inside,
 *                           -|p - t - c| outside (CollisionShape.hpp:34-38: isColliding / projectOut).  Either output may be NULL.
 *                           The device's collision kernel runs the same code and gives the same bits.
 *   admm_hip_mesh_info      triangles, BVH nodes, BVH depth, root box [lo xyz, hi xyz]; any pointer may be NULL.
 *   admm_hip_add_collision_mesh  copy the mesh into a context (before finalize: ADMM_ERR_STATE after) -> *mesh_id; the mesh may be
 *                           destroyed afterwards.  Every rank of a sharded run registers the same meshes in the same order.
 *   admm_hip_mesh_set_vertices   new positions verts [nv][3] for the same topology (nv = the count at creation): recomputes the face,
 *                           edge and vertex pseudo-normals and refits the BVH's boxes; the tree itself (built on the creation vertices)
 *                           stays, so a large deformation loosens the boxes and slows the query but never changes its result.
 *                           Refused with ADMM_ERR_ARG, the mesh left exactly as it was, for a wrong nv, a non-finite vertex, a
 *                           zero-area triangle (the lowest such original triangle named in err) or a non-positive enclosed volume.
 *                           Self-intersection is not checked: keeping the deformed mesh free of it is the caller's job.
 *                           The vertex normals' corner angles come from a libm-free acos (the same bits on the host and the device),
 *                           so an update to the creation vertices gives bit-identical closest points; the inside / outside decision
 *                           can differ from the freshly created mesh only where the pseudo-normal's dot product is within rounding of 0.
 *   admm_hip_update_collision_mesh  the same for a context's registered mesh (mesh_id of admm_hip_add_collision_mesh), verts a host
 *                           array [nv][3].  Before finalize it updates the context's copy; after it the update runs on the device, on
 *                           the context's stream, synchronously, writing in place (captured graphs stay valid) with the same bits as
 *                           admm_hip_mesh_set_vertices; a refused update (ADMM_ERR_ARG, admm_hip_last_error) leaves the live mesh
 *                           intact.  Every rank of a sharded run applies the same updates: no collective is needed, and a refusal is
 *                           the same on every rank.                                                                                 */
typedef struct admm_hip_mesh admm_hip_mesh;
int  admm_hip_mesh_create(admm_hip_mesh **out, int nv, const double *verts, int nt, const int32_t *tris, char *err, int err_len);
void admm_hip_mesh_destroy(admm_hip_mesh *mesh);
int  admm_hip_mesh_query(const admm_hip_mesh *mesh, const double t[3], int64_t n_pts, const double *pts, double *proj, double *sdist);
int  admm_hip_mesh_info(const admm_hip_mesh *mesh, int *n_tris, int *n_nodes, int *depth, double *box);
int  admm_hip_add_collision_mesh(admm_hip_ctx *ctx, const admm_hip_mesh *mesh, int *mesh_id);
int  admm_hip_mesh_set_vertices(admm_hip_mesh *mesh, int nv, const double *verts, char *err, int err_len);
int  admm_hip_update_collision_mesh(admm_hip_ctx *ctx, int mesh_id, int nv, const double *verts);
/* Body surfaces and mesh owners.  Extension, no reference counterpart (the reference collides simulated nodes only with shapes that
 * are not simulated).  A body surface is a closed triangle mesh whose vertices are simulated nodes: an ordinary registered mesh
 * (mesh_id, named as ADMM_SHAPE_MESH { 0, 0, 0, mesh_id }, the same list order and projection rule as an obstacle) that
 *   - follows its nodes: at the start of every admm_hip_step, before the explicit forces, the device reads its vertices from the
 *     frame-start x and updates it in place with the arithmetic of admm_hip_update_collision_mesh; it stays frozen for the frame's
 *     ADMM iterations.  No read-back: a frame whose positions the update would refuse (non-finite vertex, zero-area triangle,
 *     non-positive volume) keeps the last good surface, is counted, and the step returns ADMM_OK;
 *   - has an owner, its node range: the collision elements of those nodes skip the mesh (every interior node is inside its own body).
 * Edge-edge contact is out of scope (open surfaces: the thick-shell section below; self-collision within one body: admm_hip_set_body_self_collision, further below).  Friction against a body surface:
 * admm_hip_set_body_surface_friction below; it acts on the node in contact, and the surface's own nodes feel its reaction only with a
 * share set by admm_hip_set_surface_reaction (two-way contact, at the end of this file).
 *   admm_hip_add_body_surface  before finalize; tris [n_tris][3] are global node ids, all inside [node_first, node_first + node_count).
 *                           Vertices: the distinct referenced nodes in ascending id order, at their current positions (admm_hip_add_nodes
 *                           / admm_hip_set_x); triangles in the given order, renumbered.  Validated like admm_hip_mesh_create, with the
 *                           same messages.  Also sets the owner to the same range.  -> *mesh_id
 *   admm_hip_set_collision_mesh_owner  before finalize; any registered mesh; node_count 0 clears the owner.  Owner ranges of two meshes
 *                           are equal or disjoint.
 *   admm_hip_get_body_surface_status  after finalize: frame-start updates applied and refused so far, and the lowest bad triangle of
 *                           the last refusal (-1: none).
 *   admm_hip_collision_mesh_copy  a standalone copy of a registered mesh as registered (destroy with admm_hip_mesh_destroy).
 * ADMM_ERR_ARG (admm_hip_last_error): node ids or a range outside the nodes, an open / non-manifold / inward surface, overlapping owner
 * ranges, admm_hip_update_collision_mesh on a body surface, a body surface named with a nonzero translation (admm_hip_set_collision_shapes
 * or finalize); ADMM_ERR_STATE: a call in the wrong phase.  Every rank of a sharded run registers the same surfaces in the same order;
 * both shard modes hold the full frame-start x on every rank, so nothing of them goes over the collectives.                          */
int  admm_hip_add_body_surface(admm_hip_ctx *ctx, int node_first, int node_count, int n_tris, const int32_t *tris, int *mesh_id);
int  admm_hip_set_collision_mesh_owner(admm_hip_ctx *ctx, int mesh_id, int node_first, int node_count);
int  admm_hip_get_body_surface_status(admm_hip_ctx *ctx, int mesh_id, int64_t *updated, int64_t *refused, int *last_bad_tri);
int  admm_hip_collision_mesh_copy(admm_hip_ctx *ctx, int mesh_id, admm_hip_mesh **out);

/* ---- Coulomb friction at collision contacts -------------------------------------------------------------------------------------
 * Extension, no reference counterpart (the reference's contacts are frictionless).  Every entry q of the shape list carries a
 * coefficient mu_q >= 0, default 0.  In the collision projection the candidate is p = Dx + u; at a resting contact u is the contact
 * impulse over the weight, so the depth by which a shape pushes p out is the normal force, and the tangential part of p' - x0
 * (x0: the node's position at the start of the frame) is the tangential force plus the slip.  After shape q moved the point from p to
 * p' -- exactly when and how it does without friction -- and mu_q > 0:
 *     d = p' - p,  depth = |d| (0: nothing happens),  n = d / depth,  r = p' - x0,  t = r - (r.n) n,  lim = mu_q depth
 *     |t| <= lim:  p' <- p' - t              stick: tangentially back where the frame started
 *     else      :  p' <- p' - (lim / |t|) t  slip: pulled back by the cone's radius
 * and the next shape of the list starts from the new p'.  mu = +inf always sticks.  The result is not projected onto the shape again: on
 * a curved surface it sits off the surface by O(|t|^2 / R), which the next ADMM iteration corrects.  By default obstacles count as at
 * rest; "friction against moving obstacles" below gives them a motion.  An entry that names a body surface takes no coefficient from this
 * list (the surface's own: admm_hip_set_body_surface_friction).
 *   admm_hip_set_collision_friction  mu [n_shapes], n_shapes = the length of the current list; before or after finalize, between frames.
 *                           ADMM_ERR_ARG (admm_hip_last_error names the entry): a negative or NaN coefficient, another count, a nonzero
 *                           coefficient on a body-surface entry (also checked at finalize, and by admm_hip_set_collision_shapes after
 *                           it).  admm_hip_set_collision_shapes keeps the coefficients when the list's length is unchanged and zeroes
 *                           them when it changes.  With every coefficient 0 the collision batches launch exactly the frictionless
 *                           kernels; with any above 0 they launch the friction form, which also gathers x0 (admm_hip_step: the frame's
 *                           start; admm_hip_local_step_only / _dx: x as added or as admm_hip_set_x left it).  The values change under a
 *                           captured graph like shape parameters; a change between the two cases drops the graphs, which are captured
 *                           again.  Every rank of a sharded run sets the same values (both shard modes hold the full frame-start x): no
 *                           collective is involved.
 *   admm_hip_friction_query  host evaluation of the rule for n cases: p, p_out (= p'), x0 [n][3], mu [n] -> result [n][3] (p' after
 *                           friction) and mode [n]: 0 none (mu == 0 or depth == 0: result = p_out), 1 stick, 2 slip.  Either output
 *                           may be NULL.  The device's kernel runs the same code and gives the same bits.                            */
int  admm_hip_set_collision_friction(admm_hip_ctx *ctx, int n_shapes, const double *mu);
int  admm_hip_friction_query(int64_t n, const double *p, const double *p_out, const double *x0, const double *mu, double *result, int32_t *mode);

/* ---- friction against moving obstacles and body surfaces ---------------------------------------------------------------------------
 * Extension, no reference counterpart.  Moving a shape or a mesh between frames (admm_hip_set_collision_shapes,
 * admm_hip_update_collision_mesh) does not by itself tell the friction rule that the obstacle moves.  With the displacement w of the
 * obstacle's surface over the frame at the contact, one line of the rule above changes:   r = (p' - x0) - w   (per component, in that
 * order); stick then means tangentially where the node would be had it ridden on the surface for the frame.  w = 0 gives the same bits.
 * w has two sources, both zero by default and both evaluated at the contact c = p' (where the shape put the point, world coordinates):
 *   rigid motion of a list entry, nine doubles { a (linear velocity), om (angular velocity), o (pivot) }, any entry type:
 *       e = c - o;   x = (om1 e2 - om2 e1,  om2 e0 - om0 e2,  om0 e1 - om1 e0), each a difference of two rounded products;
 *       w_rigid_j = dt * (a_j + x_j)                                   dt: the context's timestep
 *   per-vertex velocities of a mesh, interpolated at the hit with the barycentric weights b of the closest point on the winning triangle
 *   (vertex region: 1 on that corner; edge: (1 - t, t); face: (1 - sv - sw, sv, sw) with 1 - sv - sw = (1 - sv) - sw; t, sv, sw the
 *   expressions of the closest-point routine), the corners' vertex ids in the triangle's canonical order (lowest vertex id first):
 *       vi_j = b0 va_j + (b1 vb_j + b2 vc_j);   w_vertex_j = dt * vi_j
 *   an entry whose mesh has vertex velocities:  w_j = w_rigid_j + w_vertex_j;  every other entry:  w = w_rigid.
 * All of it without fused multiply-adds, the same on the host and the device.
 *   admm_hip_set_collision_motion  motion [n_shapes][9], n_shapes = the length of the current list; before or after finalize, between
 *                           frames.  ADMM_ERR_ARG (the entry named): another count, a non-finite value, a nonzero motion on an entry that
 *                           names a body surface (also checked at finalize and, for kept motions, by admm_hip_set_collision_shapes).
 *                           admm_hip_set_collision_shapes keeps the motions when the list's length is unchanged and zeroes them when it
 *                           changes, as it does the coefficients.
 *   admm_hip_set_collision_mesh_velocity  vel [nv][3] for a registered obstacle mesh, after finalize (ADMM_ERR_STATE before), between
 *                           frames; NULL clears them (nv is then ignored).  ADMM_ERR_ARG: another nv, a non-finite value (the vertex
 *                           named), a body surface.  The first call for a mesh allocates its device buffer and drops the captured graphs;
 *                           admm_hip_step never allocates.
 *   admm_hip_set_body_surface_friction  the coefficient mu >= 0 (+inf allowed) of a body surface, a property of the body: it applies to
 *                           every entry that names the surface; before or after finalize.  ADMM_ERR_ARG on a mesh that is not a body
 *                           surface or a negative / NaN mu.  The surface's vertex velocities are its nodes' frame-start v (before the
 *                           explicit forces), gathered beside its vertices at the start of every admm_hip_step; a refused frame keeps the
 *                           last good surface and the velocities that went with it; admm_hip_local_step_only / _dx use both as finalize
 *                           (v = 0) or the last admm_hip_step left them.  One-sided like the push itself: the node in contact feels the
 *                           friction, the surface's nodes no reaction; two bodies that list each other's surfaces get friction both ways.
 * The collision batches launch the moving form of the friction kernel when an entry with mu > 0 has a nonzero motion or a mesh with
 * velocities set, or a body surface named in the list has a coefficient above 0; otherwise exactly what they launched before (the same
 * bits).  The values live in device memory and change under a captured graph; a call that changes the launched kernels drops the graphs.
 * Every rank of a sharded run makes the same calls (both shard modes hold the full frame-start x and v): no collective is involved.
 *   admm_hip_friction_query_moving  admm_hip_friction_query with w [n][3]; the same bits as the device.
 *   admm_hip_mesh_velocity_query    host evaluation of the interpolation for n points q [n][3] against the instance translated by t[3]:
 *                           out [n][3] = vi at the closest point (vel [nv][3]; may be NULL with out), weights [n][3] = b, corner_ids
 *                           [n][3] = the winning triangle's vertex ids; any output may be NULL.  The same bits as the device.        */
int  admm_hip_set_collision_motion(admm_hip_ctx *ctx, int n_shapes, const double *motion);
int  admm_hip_set_collision_mesh_velocity(admm_hip_ctx *ctx, int mesh_id, int nv, const double *vel);
int  admm_hip_set_body_surface_friction(admm_hip_ctx *ctx, int mesh_id, double mu);
int  admm_hip_friction_query_moving(int64_t n, const double *p, const double *p_out, const double *x0, const double *w, const double *mu, double *result, int32_t *mode);
int  admm_hip_mesh_velocity_query(const admm_hip_mesh *mesh, int64_t n, const double *q, const double t[3], const double *vel, double *out, double *weights, int32_t *corner_ids);

/* ---- oriented obstacles: a rigid frame per list entry, and a box --------------------------------------------------------------------
 * Extension, no reference counterpart.  Every entry q of the shape list carries a frame of twelve doubles { R (3x3, row-major), o (pivot) },
 * default the identity about the origin: the entry's shape, exactly as its params describe it, rotated by R about o.  For an entry whose R
 * is not exactly the identity, in every collision kernel:
 *     e = p - o;    q_j = o_j + (R_0j e_0 + (R_1j e_1 + R_2j e_2))          the candidate in local coordinates, q = o + R^T (p - o)
 *     the entry's unframed rule runs on q (for a mesh: the box test, closest point and inside test with the translation t) -> q'
 *     only if that moved the point:   e = q' - o;   p'_j = o_j + (R_j0 e_0 + (R_j1 e_1 + R_j2 e_2))           p' = o + R (q' - o)
 * every product rounded, the sums associated as written, no fused multiply-adds, the same on the host and the device.  A point the shape
 * did not move keeps its bits (no round trip).  Friction and its moving form then run on the world-space p, p', x0 and w unchanged; the
 * interpolated vertex velocity vi of a framed mesh is in the mesh's own coordinates and is rotated first, vi'_j = R_j0 vi_0 + (R_j1 vi_1 +
 * R_j2 vi_2), before w_vertex = dt vi'.  Turning a frame between frames does not by itself tell the friction rule that the obstacle
 * moves: admm_hip_set_collision_motion does (its pivot and angular velocity are in world coordinates).
 * ADMM_SHAPE_BOX { hx, hy, hz, - }: half extents > 0, the box centred at its frame's pivot o (the origin without a frame; for the box the
 * pivot counts even when R is the identity), axes along the local coordinate axes.  With d = q - o and depth_j = h_j - |d_j|: the point
 * collides exactly when all three depths are > 0, and moves to the face of least depth (ties: the lowest axis), to o_j + h_j when d_j >= 0
 * and to o_j - h_j otherwise; the other two coordinates are untouched.
 *   admm_hip_set_collision_frames  frames [n_shapes][12], n_shapes = the length of the current list; NULL: every entry back to the identity.
 *                           Before or after finalize, between frames.  ADMM_ERR_ARG (admm_hip_last_error names the entry): another count,
 *                           a non-finite value, an R that is not a rotation (an element of R^T R - I, or det R - 1, beyond 1e-12 in
 *                           size), a non-identity R on an entry that names a body surface (also checked at finalize and, for kept frames,
 *                           by admm_hip_set_collision_shapes).  A refused call leaves the frames as they were.
 *                           admm_hip_set_collision_shapes keeps the frames when the list's length is unchanged and resets them when it
 *                           changes, as it does the coefficients and motions; it refuses (ADMM_ERR_ARG, the entry named) a box whose half
 *                           extents are not positive and finite.
 * A list with a non-identity R or a box launches the framed form of the collision kernel for its collision batches, a launch of their own
 * in both launch modes; every other list launches exactly what it launched before (the same bits).  The values live in device memory and
 * change under a captured graph; a call that changes the launched kernels drops the graphs.  Every rank of a sharded run makes the same
 * calls: no collective is involved.
 *   admm_hip_shape_query    host evaluation of one analytic entry (floor, sphere, cylinder, box; ADMM_ERR_ARG for a mesh, bad half extents
 *                           or a bad frame) with its frame (NULL: none) for n points p [n][3]: out [n][3] = the point after the entry,
 *                           moved [n] = 1 where the entry moved it.  Either output may be NULL.  The same bits as the device.
 *   admm_hip_mesh_query_framed  admm_hip_mesh_query for an instance with a frame: proj in world coordinates, sdist as measured in local
 *                           coordinates.  frame NULL (or the identity): the bits of admm_hip_mesh_query.                               */
int  admm_hip_set_collision_frames(admm_hip_ctx *ctx, int n_shapes, const double *frames);
int  admm_hip_shape_query(int type, const double params[4], const double *frame, int64_t n, const double *p, double *out, int32_t *moved);
int  admm_hip_mesh_query_framed(const admm_hip_mesh *mesh, const double t[3], const double *frame, int64_t n_pts, const double *pts, double *proj, double *sdist);

/* ---- open triangle surfaces as thick shells ----------------------------------------------------------------------------------------
 * Extension, no reference counterpart.  An open surface -- a sheet, a flag, a terrain patch, a half pipe, a cloth -- has no inside, so
 * the closed-mesh rule has no meaning for it.  It collides as a shell of half thickness r > 0: it occupies every point whose distance to
 * the surface is below r, and a point is pushed to distance r on the side it is currently on.  For a candidate q (relative to the entry's
 * translation t, in local coordinates under a frame), every product and sum rounded, no fused multiply-adds, in this order:
 *     1. the traversal runs only when  lo_j - r < q_j < hi_j + r  holds strictly for j = 0, 1, 2 (lo, hi: the root box); a point that
 *        fails keeps its bits;
 *     2. h = the closest point c (ties: the lowest triangle index) and its squared distance d2, from a search bounded by r * r: the
 *        hit of the closed meshes' search whenever d2 < r * r, none otherwise;
 *     3. the point collides exactly when a hit exists and  d2 < r * r;
 *     4. e_j = q_j - c_j,  d = sqrt(d2);   d > 0:  s = r / d,  p'_j = c_j + s * e_j;   d == 0:  p'_j = c_j + r * n_j  with n the unit
 *        normal of the winning triangle;
 *     5. p_j = t_j + p'_j, then under a frame to_world -- only for a point that was moved.
 * Everything after the push is what a closed mesh's entry does on the world-space points: the coefficient, the vertex velocities
 * interpolated at the hit, the rigid motion, the friction rule.  Without side memory (the section after the next) the rule does not know
 * the side a node started the frame on: a node that crosses the mid-surface within one frame leaves on the far side, so keep r above
 * closing speed x dt; with it keep the reach R above closing speed x dt + r.  Edge-edge contact, continuous detection, a thickness on closed meshes and reactions on a sheet's own nodes are out of scope.
 *   admm_hip_mesh_create_open   like admm_hip_mesh_create for a surface that may have boundary edges: every directed edge at most once
 *                           (edge-manifold, consistently oriented where two faces meet), no degenerate triangle, half_thickness finite
 *                           and > 0; at least one triangle.  A closed input is accepted and simply is a shell.  ADMM_ERR_ARG with the
 *                           edge or triangle named in err otherwise.  The same BVH, leaf order and topology tables as a closed mesh; a
 *                           boundary edge's pseudo-normal is its one face's normal.
 *   admm_hip_mesh_thickness     *r = the half thickness; 0 for a closed mesh.
 *   on an open mesh, admm_hip_mesh_query / _framed return  proj = the point after the rule (bitwise the input where the rule does not move
 *                           it)  and  sdist = r - d  where a triangle is nearer than r (positive: colliding), -inf where the bounded
 *                           search found none or the box test failed; admm_hip_mesh_velocity_query, admm_hip_mesh_info: unchanged;
 *                           admm_hip_mesh_set_vertices / admm_hip_update_collision_mesh refuse a wrong count, a non-finite vertex and a
 *                           zero-area triangle only (no volume condition).
 *   admm_hip_mesh_closest       the two searches as they are, for tests: r2 < 0: the unbounded one, else the one bounded by r2, for n
 *                           points q [n][3] relative to the instance: c [n][3], d2 [n], slot [n] (leaf order; -1: none), reg [n] (the
 *                           feature: 0 face, 1-3 edges, 4-6 vertices), tri [n] (the original triangle).  Any output may be NULL.
 *   admm_hip_add_collision_mesh accepts an open mesh; an ADMM_SHAPE_MESH entry names it like any other.  A list that names an open mesh
 *                           makes the collision batches launch project_collision_shell_kernel; a list that names none launches exactly
 *                           what it launched before.  Only admm_hip_set_collision_shapes can change that; it drops the captured graphs then.
 *   admm_hip_set_collision_mesh_thickness  a registered open mesh's half thickness, before or after finalize, between frames; it lives in a
 *                           device table and changes under a captured graph like a shape parameter.  ADMM_ERR_ARG: a closed mesh, r not
 *                           finite or not > 0.
 *   admm_hip_add_sheet_surface  admm_hip_add_body_surface for an open surface of simulated nodes, such as a cloth: the same vertex
 *                           numbering, owner range, frame-start update (verdict on the device, counted in the status, a refused frame
 *                           keeps the last good surface; no volume condition) and refusals (a per-entry coefficient, a translation, a
 *                           frame, admm_hip_update_collision_mesh); admm_hip_get_body_surface_status and
 *                           admm_hip_set_body_surface_friction apply to it.  Its own nodes skip it unless
 *                           admm_hip_set_sheet_self_collision says otherwise (the next section).                                        */
int  admm_hip_mesh_create_open(admm_hip_mesh **out, int nv, const double *verts, int nt, const int32_t *tris, double half_thickness, char *err, int err_len);
int  admm_hip_mesh_thickness(const admm_hip_mesh *mesh, double *r);
int  admm_hip_mesh_closest(const admm_hip_mesh *mesh, int64_t n, const double *q, double r2, double *c, double *d2, int32_t *slot, int32_t *reg, int32_t *tri);
int  admm_hip_set_collision_mesh_thickness(admm_hip_ctx *ctx, int mesh_id, double half_thickness);
int  admm_hip_add_sheet_surface(admm_hip_ctx *ctx, int node_first, int node_count, int n_tris, const int32_t *tris, double half_thickness, int *mesh_id);

/* ---- a sheet surface that collides with itself: cloth self-collision ------------------------------------------------------------------
 * Extension, no reference counterpart.  By default the collision elements of a sheet surface's own nodes skip the surface.  With
 * self-collision switched on they do not: node i of the sheet, which is vertex vi of the surface (the numbering of
 * admm_hip_add_sheet_surface: the referenced nodes in ascending order, vi = i - node_first when every node of the range is referenced),
 * runs the shell rule above, steps 1 to 5, every product and sum rounded, no fused multiply-adds, with one change in step 2:
 *     2'. the bounded search ignores every triangle that has vi as a corner (the node's 1-ring); among the remaining triangles the winner
 *         is the minimum of (d2, original triangle index), compared lexicographically, with d2 < r * r.  The BVH only prunes, so the
 *         result does not depend on its shape.
 * Everything else is the shell rule: the decision d2 < r * r, the push to distance r on the side the point is on (d == 0: along the
 * winning face's normal), the translation, and everything after the push -- the surface's own coefficient
 * (admm_hip_set_body_surface_friction), the frame-start v of the winning triangle's nodes interpolated at the hit, the friction rule.
 * Nodes that do not belong to the sheet meet it exactly as before.  The surface is frozen at the frame-start x for the frame's
 * iterations: a node meets where the rest of the cloth was at the start of the frame.  Contact is vertex-triangle outside a node's
 * 1-ring only: edge-edge contact, side memory for the sheet's own nodes and continuous detection are out of scope (a closed body surface: the section after the next), and
 * the push is one-sided (the winning triangle's nodes feel no reaction).
 *   admm_hip_set_sheet_self_collision  before finalize (ADMM_ERR_STATE after it); on != 0 switches it on for the sheet surface mesh_id.
 *                           ADMM_ERR_ARG, naming the mesh, for an obstacle mesh or a closed body surface (admm_hip_set_body_self_collision is its call).  The collision batches of a
 *                           list that names such a sheet launch project_collision_self_kernel; a context where no sheet self-collides
 *                           launches exactly what it launched before.
 *   admm_hip_finalize       refuses (ADMM_ERR_ARG, naming the vertex, the triangle and the distance) a self-colliding sheet in whose
 *                           positions a vertex lies nearer than r to a triangle it is not a corner of: every such node would be pushed by
 *                           its own neighbourhood from the first frame.  On a regular grid of spacing h this bounds r below roughly
 *                           0.7 h.  Two self-colliding sheets over the same node range are refused too.
 *   admm_hip_mesh_query_excluding  the context-free host evaluation of the rule with a per-point excluded vertex, the same bits as the
 *                           device: admm_hip_mesh_query_framed on an open mesh with step 2'; tri [n] = the winning original triangle (-1:
 *                           none nearer than r).  frame NULL: the identity; skip_vertex NULL or skip_vertex[i] = -1: nothing is left out,
 *                           the bits of admm_hip_mesh_query_framed.  ADMM_ERR_ARG on a closed mesh (admm_hip_mesh_create) and for a
 *                           skip_vertex outside [-1, nv).  Any output may be NULL.
 *   admm_hip_mesh_velocity_query_excluding  admm_hip_mesh_velocity_query at the hit of that search (q, t as there); a point with no
 *                           triangle nearer than r outside the excluded 1-ring gets zeros and corner ids -1.                            */
int  admm_hip_set_sheet_self_collision(admm_hip_ctx *ctx, int mesh_id, int on);
int  admm_hip_mesh_query_excluding(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *skip_vertex, const double t[3], const double *frame,
                                   double *proj, double *sdist, int32_t *tri);
int  admm_hip_mesh_velocity_query_excluding(const admm_hip_mesh *mesh, int64_t n, const double *q, const int32_t *skip_vertex, const double t[3], const double *vel,
                                            double *out, double *weights, int32_t *corner_ids);

/* ---- side memory for thick shells: fast nodes do not tunnel ---------------------------------------------------------------------------
 * Extension, no reference counterpart.  An open mesh may be given a reach R, finite, R >= r > 0; it then has side memory: for every node
 * and every such mesh the context keeps one int32 side s: +1 the side the surface's normals point to, -1 the other one, 0 none.  For a
 * hit h of a point q (relative to the entry's translation, in local coordinates under a frame), every product and sum rounded, no fused
 * multiply-adds:
 *     g = (q0 - c0) n0 + (q1 - c1) n1 + (q2 - c2) n2,  n the pseudo-normal of the hit's feature;  side_of = +1 for g > 0, -1 for g < 0, else 0;
 *     a boundary hit: the hit's feature is a boundary edge or a vertex incident to one.
 * Latch, once per frame from the frame-start position, first in admm_hip_step (after the body surfaces' update, before the explicit
 * forces).  A node whose body owns the mesh is skipped (its side stays 0).  Any other node, previous side s; the first step whose
 * condition holds decides:
 *     1. the box test of the shell rule with R in place of r fails: s' = 0;
 *     2. the search bounded by R * R finds nothing: s' = 0;
 *     3. a boundary hit: s' = 0 (a node that goes round the rim forgets);
 *     4. s != 0: s' = s (sticky: a frame that ended on the wrong side does not relearn it);
 *     5. s == 0: s' = side_of(q, h) when d2 >= r * r, else 0 (never learned from inside the shell).
 * Projection, per iteration, for an entry that names such a mesh.  A node with s == 0 runs the shell rule as it stands (a self-colliding
 * sheet's own node with its 1-ring left out).  A node with s != 0:
 *     1. the box test with R fails: the point keeps its bits;       2. the search bounded by R * R finds nothing: it keeps its bits;
 *     3. a boundary hit, or side_of(q, h) * s >= 0 (or d2 == 0): the unsigned rule on this hit -- it collides iff d2 < r * r, step 4 of the shell rule;
 *     4. otherwise the node has crossed: d = sqrt(d2), sc = r / d, e_j = q_j - c_j, p'_j = c_j - sc * e_j (mirrored through the closest
 *        point to distance r on the remembered side);
 *     5. p_j = t_j + p'_j, then under a frame to_world -- only for a point that was moved.
 * Everything after the push is unchanged.  Keep R above closing speed x dt + r; the traversal is bounded by R instead of r.  A
 * self-colliding sheet's own nodes keep the unsigned rule: in the flat parts of a cloth the nearest triangle outside the 1-ring lies in
 * the node's own plane, so the sign there would be noise.  Both shard modes hold the full frame-start x on every rank, so every rank
 * latches every node from the same bits and nothing new crosses a collective.
 *   admm_hip_set_collision_mesh_side_memory  before finalize (ADMM_ERR_STATE after it); reach = 0 switches memory off.  ADMM_ERR_ARG,
 *                           naming the mesh, for a closed mesh, a non-finite reach or one below the mesh's half thickness.
 *                           admm_hip_set_collision_mesh_thickness then refuses r > reach; finalize and admm_hip_set_collision_shapes
 *                           refuse a list that names such a mesh in two entries (a node has one side per mesh).  A list that names one
 *                           launches project_collision_sided_kernel (collision form 6); a context without one uploads and launches
 *                           exactly what it did.
 *   admm_hip_get_collision_sides / admm_hip_set_collision_sides  after finalize: n_nodes values in the caller's node order for one mesh with
 *                           memory; values outside {-1, 0, 1} are refused.  The sides are part of a checkpoint beside x, v and u.
 *   admm_hip_latch_collision_sides  exactly the launches admm_hip_step begins with (body surfaces, then the latch) from the current x,
 *                           synchronised: for callers that teleport nodes with admm_hip_set_x, and for tests.
 *   admm_hip_reset_collision_sides  zeroes all sides.  admm_hip_set_x and admm_hip_set_collision_shapes leave them alone (a translation
 *                           changed between frames is the moving-obstacle case).
 *   admm_hip_mesh_side_latch, admm_hip_mesh_query_sided  the context-free host evaluations, the device's bits (prev / side NULL: all 0;
 *                           frame NULL: the identity).  query_sided: sdist = r - d for an unsigned push, r + d for a crossed one, -inf for
 *                           none; tri = the winning original triangle of a push; crossed = 1 where step 4 ran; with side all zero the
 *                           bits of admm_hip_mesh_query_framed.  ADMM_ERR_ARG on a closed mesh, a reach not finite or below r, a side
 *                           outside {-1, 0, 1}.  admm_hip_mesh_velocity_query at the hit needs no sibling: the hit is the unbounded search's.
 *   admm_hip_mesh_boundary_table  for tests: per leaf slot the bits (bit reg, 1..6, set for a boundary feature) and the original triangle.
 *   admm_hip_mesh_feature_normal  for tests: the stored pseudo-normal [n][3] of n (slot, reg) pairs of admm_hip_mesh_closest: the n of g.      */
int  admm_hip_set_collision_mesh_side_memory(admm_hip_ctx *ctx, int mesh_id, double reach);
int  admm_hip_get_collision_sides(admm_hip_ctx *ctx, int mesh_id, int32_t *side);
int  admm_hip_set_collision_sides(admm_hip_ctx *ctx, int mesh_id, const int32_t *side);
int  admm_hip_latch_collision_sides(admm_hip_ctx *ctx);
int  admm_hip_reset_collision_sides(admm_hip_ctx *ctx);
int  admm_hip_mesh_side_latch(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *prev, double reach, const double t[3], const double *frame,
                              int32_t *side_out);
int  admm_hip_mesh_query_sided(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *side, double reach, const double t[3], const double *frame,
                               double *proj, double *sdist, int32_t *tri, int32_t *crossed);
int  admm_hip_mesh_boundary_table(const admm_hip_mesh *mesh, int32_t *bits, int32_t *orig);
int  admm_hip_mesh_feature_normal(const admm_hip_mesh *mesh, int64_t n, const int32_t *slot, const int32_t *reg, double *out);

/* ---- self-collision of a closed body surface: a tet body meets its own skin ---------------------------------------------------------------
 * Extension, no reference counterpart.  A body surface's own nodes skip it, which is right for interior nodes and wrong for surface
 * nodes: a bar bent back on itself, the jaws of a gripper, an arm and its torso pass through each other.  A body surface S
 * (admm_hip_add_body_surface) may be given three lengths: a half gap r > 0, a reach R >= r, a rest radius rho >= R.  X are the surface's
 * vertices as admm_hip_add_body_surface registered them, the rest shape; the context keeps a copy and later updates do not change it.
 * Node i of the body has a candidate q; a body surface has no translation and no frame.  An interior node (no vertex of S) skips S as
 * before.  A surface node, vertex vi of S, every product and sum rounded, no fused multiply-adds:
 *     1. the box test of the shell rule with R (lo_j - R < q_j < hi_j + R strictly, the root box) fails: the point keeps its bits;
 *     2. the winner is the minimum of (d2, original triangle index), d2 < R * R, over the triangles that are not rest-near vi.  Triangle
 *        T with corners a, b, c = cid[3 orig + 0..2], in that order, is rest-near when the closest point of {X[a], X[b], X[c]} to X[vi]
 *        gives e0 * e0 + e1 * e1 + e2 * e2 < rho * rho; the 1-ring is rest-near by construction.  A left-out triangle never tightens
 *        the bound and the boxes only prune with the usual margin, so the result does not depend on the tree.  The test is evaluated
 *        lazily, for a triangle whose d2 would make it the new best; the winner and its bits are the definition's.  No hit: the point
 *        keeps its bits;
 *     3. g = (q0 - c0) n0 + (q1 - c1) n1 + (q2 - c2) n2, n the pseudo-normal of the hit's feature.  g >= 0 or d2 == 0: the unsigned rule
 *        on this hit -- it collides iff d2 < r * r, then step 4 of the shell rule.  g < 0: the node has crossed the skin and is mirrored
 *        to distance r outside, d = sqrt(d2), p'_j = c_j - (r / d)(q_j - c_j);
 *     4. everything after the push is unchanged: the surface's own coefficient (admm_hip_set_body_surface_friction), the frame-start v
 *        of the winning triangle's nodes interpolated at the hit, the rigid displacement, the friction rule.
 * Nodes of other bodies meet S by the closed-mesh rule, exactly as before.  The surface is frozen at the frame-start x; contact is
 * one-sided and vertex-triangle, like every surface here.  Keep R above closing speed x dt + r, rho above R by the compression the body
 * is expected to see, and rho below the body's thinnest part, or the two faces of a thin plate never see each other.  Both shard modes
 * hold the full frame-start x on every rank; nothing new crosses a collective.
 *   admm_hip_set_body_self_collision  before finalize (ADMM_ERR_STATE after it); r = 0 switches it off.  ADMM_ERR_ARG, naming the mesh,
 *                           for an obstacle mesh, a sheet surface, a non-finite value, reach < r, rest_radius < reach.  Finalize refuses
 *                           (ADMM_ERR_ARG naming vertex, triangle and distance) a body in whose finalize positions the rule would already
 *                           move one of its own vertices, and two self-colliding surfaces (sheets or bodies) over one node range: a
 *                           node has one vertex id.  A list that names such a surface launches project_collision_bodyself_kernel
 *                           (collision form 7); a context where no body self-collides uploads and launches exactly what it did.
 *   admm_hip_mesh_query_self  the context-free host evaluation, the device's bits: point i is vertex vertex_id[i] of the closed mesh
 *                           (-1: skipped, proj = the point, tri = -1), rest_verts [nv][3] the rest shape.  sdist = r - d for a hit on the
 *                           outside (> 0: pushed; <= 0: a hit within the reach that leaves the point alone), r + d for a crossed one,
 *                           -inf for no hit; tri = the winning original triangle of a hit (-1: none); crossed = 1 where the mirror ran.  ADMM_ERR_ARG on an open mesh, for an id outside [-1, nv) and for lengths the setter
 *                           refuses (r = 0 included).
 *   admm_hip_mesh_velocity_query_self  admm_hip_mesh_velocity_query at the hit of that search (no other call evaluates at a given
 *                           triangle); a point without a hit within the reach gets zeros and corner ids -1.                            */
int  admm_hip_set_body_self_collision(admm_hip_ctx *ctx, int mesh_id, double r, double reach, double rest_radius);
int  admm_hip_mesh_query_self(const admm_hip_mesh *mesh, int64_t n_pts, const double *pts, const int32_t *vertex_id, const double *rest_verts, double r, double reach,
                              double rest_radius, double *proj, double *sdist, int32_t *tri, int32_t *crossed);
int  admm_hip_mesh_velocity_query_self(const admm_hip_mesh *mesh, int64_t n, const double *q, const int32_t *vertex_id, const double *rest_verts, double reach,
                                       double rest_radius, const double *vel, double *out, double *weights, int32_t *corner_ids);

/* ---- multi-GPU ------------------------------------------------------------
 * Elements shard across ranks (see admm_hip_set_shard_mode); must be called before finalize.  The hook must sum `count`
 * doubles of a DEVICE buffer in place across the ranks (an all-reduce), ordered on `stream`; every rank makes the same
 * calls in the same order, buffers and counts differ between calls: per ADMM iteration once (contiguous shards: the
 * whole right-hand side; subtree shards: the top rows) or twice (distributed top: also the top's x), once per frame
 * (subtree shards: the full x), and inside admm_hip_finalize / admm_hip_recompute_weights under rank-local factorization
 * (admm_hip_set_factor_local).  No reference counterpart (the reference is single-process).   */
typedef int (*admm_hip_allreduce_fn)(void *user, void *dev_buf, int64_t count, void *hip_stream);
int admm_hip_set_shard(admm_hip_ctx *ctx, int rank, int world);
int admm_hip_set_allreduce(admm_hip_ctx *ctx, admm_hip_allreduce_fn fn, void *user);
/* Transports that only see HOST memory (MPI without GPU support, shared memory between the ranks of one node -- see
 * host/admm/Comm.hpp ShmAllReduce): the library stages the buffer through pinned host memory around fn, which must sum
 * host_buf[0..count) in place across the ranks.  Replaces any device hook; NULL removes it.                          */
typedef int (*admm_hip_host_allreduce_fn)(void *user, double *host_buf, int64_t count);
int admm_hip_set_host_allreduce(admm_hip_ctx *ctx, admm_hip_host_allreduce_fn fn, void *user);
/* RCCL inside the library (north_star: "host stays C++"): with a communicator installed the per-iteration exchange is
 * ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, <the context's stream>) issued by the step loop itself -- no
 * host hook between the kernels, and (ADMM_HIP_GRAPH_COMM=1) the whole multi-GPU iteration replays as one HIP graph.
 * librccl.so is bound at run time with dlopen (the copy already loaded in the process first, e.g. PyTorch's; env
 * ADMM_HIP_RCCL_LIB overrides); single-GPU users never load it.
 *   admm_hip_rccl_unique_id  rank 0: 128 bytes (ncclUniqueId) to hand to every rank by whatever means the host has
 *   admm_hip_rccl_init       every rank, collectively: ncclCommInitRank on the context's device; the library owns the communicator
 *   admm_hip_set_rccl_comm   use an ncclComm_t the caller already has (not owned; NULL = back to the hook)
 *   admm_hip_debug_allreduce one checked all-reduce of a caller-owned device buffer through whatever is installed
 *   admm_hip_rccl_async_error  ncclCommGetAsyncError of the installed communicator: *nccl_result = 0 (ncclSuccess) while the
 *                            communicator is healthy; a non-zero value also makes the call return ADMM_ERR_COMM with the RCCL
 *                            error text in admm_hip_last_error.  admm_hip_step polls it once per frame when a communicator is
 *                            installed, so a peer that died surfaces as a failed step instead of a silent hang in the next sync.
 *                            No communicator installed: *nccl_result = 0, ADMM_OK.                                             */
int admm_hip_rccl_unique_id(void *id128);
int admm_hip_rccl_init(admm_hip_ctx *ctx, const void *id128, int rank, int world);
int admm_hip_set_rccl_comm(admm_hip_ctx *ctx, void *nccl_comm);
int admm_hip_debug_allreduce(admm_hip_ctx *ctx, void *dev_buf, int64_t count);
int admm_hip_rccl_async_error(admm_hip_ctx *ctx, int *nccl_result);
/* A short HOST vector summed in place across the ranks through the same transport (no-op at world 1).  The class mirror uses
 * it for what the reference keeps per force object and a sharded run keeps on the owner rank only: a released MovingAnchor's
 * position, point->pos = Dx of the last project() (AnchorForce.cpp:80-83) -- owner's value, zeros elsewhere.              */
int admm_hip_allreduce_host(admm_hip_ctx *ctx, double *host_buf, int64_t count);
/* How the work is split across the ranks (before finalize; env ADMM_HIP_SHARD=contiguous|subtree overrides):
 *   ADMM_SHARD_CONTIGUOUS  every batch is cut into `world` contiguous element ranges; per ADMM iteration the whole right-hand
 *                          side (3 n doubles) is all-reduced and every rank runs the complete solve.
 *   ADMM_SHARD_SUBTREE     the elimination tree is cut below its top: every rank owns whole subtrees and the elements touching
 *                          them (an element's nodes lie in one subtree plus separators above it: a user force whose nodes lie
 *                          in two ranks' subtrees is refused at finalize with ADMM_ERR_UNSUPPORTED); per iteration ONE small
 *                          all-reduce carries the top separators' partial right-hand sides and the subtree roots' contributions,
 *                          only the top levels of the solve are replicated, and the full x is rebuilt once per frame.  With
 *                          2 / 4 / 8 / 16 ranks and >= 300k nodes (ADMM_HIP_DIST_TOP) the top is ONE root supernode whose product
 *                          with its explicit inverse is split by rows across the ranks: nothing of the solve is replicated, a
 *                          second small all-reduce per iteration gathers the top's x (admm_hip_info.dist_top).
 * admm_hip_local_elements: this rank's elements of a batch (ascending reference order) -- the order of read_local / write_local. */
enum { ADMM_SHARD_CONTIGUOUS = 0, ADMM_SHARD_SUBTREE = 1 };
int admm_hip_set_shard_mode(admm_hip_ctx *ctx, int mode);
int admm_hip_local_elements(admm_hip_ctx *ctx, int batch, int32_t *ids, int capacity, int *n_local);
/* test hook: the rank that owns each node's subtree (original node order), -1 = replicated top; 0 everywhere without subtree sharding */
int admm_hip_debug_node_owner(admm_hip_ctx *ctx, int32_t *owner);
/* test hook: the supernode that holds each node's column (original node order; the number admm_hip_last_error names for a pivot that
 * is not positive), the node's column inside it (0 = the supernode's first) and every supernode's parent ([admm_hip_info.n_supernodes],
 * -1 = a root); any array may be NULL */
int admm_hip_debug_node_supernode(admm_hip_ctx *ctx, int32_t *supernode, int32_t *column, int32_t *parent);

/* ---- initialize -----------------------------------------------------------
 * replaces: System::initialize()                          (System.cpp:98-156)
 * Force::initialize + get_selector for every element (rest shape matrices,
 * weights, global_idx), assembly of A = M + dt^2 D^T W^2 D, its sparse
 * factorization (host) and the upload of every device-resident array.        */
int admm_hip_finalize(admm_hip_ctx *ctx);
/* Small systems (n_nodes <= ADMM_HIP_DENSE_MAX, default 2048; env, 0 disables): the factor is used once on the host to
 * form the dense A_s^-1 (n x n, <= 33 MB) and every solve becomes ONE kernel, x = A_s^-1 b, instead of ~2 launches per
 * elimination-tree level whose dependent latencies dominate at this size (the reference's shipped scenes have 777-1251 nodes). */

/* replaces: System::recompute_weights()                   (System.cpp:159-179)
 * after admm_hip_set_weights changed per-element weights: re-assemble, re-factor, re-upload.
 * A failure (ADMM_ERR_FACTOR "system matrix is not positive definite (supernode s)" for weights that make A_s indefinite or NaN, or an
 * error of the device) leaves no usable factor: admm_hip_step, admm_hip_solve_only, admm_hip_local_step_only and admm_hip_local_step_dx
 * then return ADMM_ERR_STATE, naming that failure, until a later admm_hip_recompute_weights succeeds.  Under rank-local factorization
 * every rank returns the same code and names the same supernode (admm_hip_set_factor_local); so does admm_hip_finalize. */
/* weights: [n_elems] (a generic batch: [n_rows], one per selector row as get_selector pushes them) */
int admm_hip_set_weights(admm_hip_ctx *ctx, int batch, const double *weights);
int admm_hip_recompute_weights(admm_hip_ctx *ctx);

/* ---- per-frame host-mutable parameters --------------------------------------
 * replaces: writes to ControlPoint::pos / ::active from callbacks
 * (AnchorForce.hpp:71-80; samples/poordillo/poordillo.cpp:196-248)           */
int admm_hip_update_anchors(admm_hip_ctx *ctx, int batch, const double *targets, const int32_t *active);
/* replaces: writes to ExplicitForce::direction (samples/windyflag/windyflag.cpp:141-152) */
int admm_hip_set_gravity(admm_hip_ctx *ctx, int which, double gx, double gy, double gz);

/* ---- step -----------------------------------------------------------------
 * replaces: System::step()                                (System.cpp:26-75)
 * one frame: explicit forces, x_bar, admm_iters x (local step, RHS, solve),
 * velocity update.  Asynchronous on the context's stream; admm_hip_sync or any
 * get_* call waits for it.  pre_step_callbacks stay on the host side
 * (host/admm/System.hpp runs them before calling this).                      */
int admm_hip_step(admm_hip_ctx *ctx, int admm_iters);
int admm_hip_sync(admm_hip_ctx *ctx);

/* ---- state access ---------------------------------------------------------
 * replaces: reads/writes of System::m_x, m_v              (System.hpp:47-49) */
int admm_hip_get_x(admm_hip_ctx *ctx, double *x);
int admm_hip_set_x(admm_hip_ctx *ctx, const double *x);
int admm_hip_get_v(admm_hip_ctx *ctx, double *v);
int admm_hip_set_v(admm_hip_ctx *ctx, const double *v);

/* The frame boundary of the class API: what host/admm/System.hpp does around admm_hip_step because m_x / m_v are
 * public members a caller may read or edit between steps (System.hpp:47-49; samples/singletet.cpp:44 writes m_x).
 * upload_state is asynchronous on the context's stream (x, v or both; NULL = leave the device copy), download_state
 * returns when both vectors have arrived.  admm_hip_pin_host page-locks (on = 1) or releases (on = 0) a caller buffer;
 * when both vectors travel and both are page-locked, ONE kernel each way addresses them directly over PCIe (linear on the
 * host side, the reordering to the factor's node order on the device side; ADMM_HIP_STATE_ZEROCOPY=0: one DMA per vector
 * + reordering kernels, also the path of pageable memory).  The caller must not touch x / v between upload_state and the
 * next synchronising call (admm_hip_download_state, admm_hip_sync): the kernel reads them asynchronously.  Systems of up to 12 288
 * nodes (ADMM_HIP_STATE_DIRECT), when both vectors travel: no DMA at all -- the vectors are copied by the host into / out of a
 * page-locked buffer of the context that the permutation kernels address directly (the DMAs' submission latency is most
 * of a small scene's frame boundary); upload_state has then read x and v when it returns.                          */
/* (a refused registration returns ADMM_ERR_HIP without touching last_error or HIP's sticky error: the caller may go on
 * with pageable memory)                                                                                               */
int admm_hip_pin_host(admm_hip_ctx *ctx, void *p, size_t bytes, int on);
int admm_hip_upload_state(admm_hip_ctx *ctx, const double *x, const double *v);
int admm_hip_download_state(admm_hip_ctx *ctx, double *x, double *v);

/* ---- parity / introspection ------------------------------------------------
 * u, z: [n_local_elems][rows] element-major (compact rows), state:
 * [n_local_elems][ADMM_KIND_STATE]; n_iters: L-BFGS outer iterations of the last
 * project (hyperelastic kinds).  Any pointer may be NULL.  Replaces the
 * protected System::curr_u / curr_z (System.hpp:98-99) and
 * HyperElasticTet::last_prox_result (TetForce.hpp:146).                      */
int admm_hip_read_local(admm_hip_ctx *ctx, int batch, double *u, double *z, double *state, int32_t *n_iters);
/* z of the tet batches is an output nobody reads back in a plain frame -- every project() overwrites it from Dx + u (the
 * reference's curr_z is a protected member, System.hpp:98-99).  admm_hip_keep_z(ctx, 0) stops admm_hip_step from storing
 * it (72 bytes per tet and ADMM iteration less; what host/admm/System.hpp and bench.py do); read_local's z is then the
 * value of the last call that kept it.  Default: kept.  The parity entry points below and residual tracking always keep it. */
int admm_hip_keep_z(admm_hip_ctx *ctx, int on);
int admm_hip_write_local(admm_hip_ctx *ctx, int batch, const double *u, const double *state);
/* rest data computed by Force::initialize: weight [n], rest [n][12] (tets: B 4x3
 * col-major; tris: B 3x2 in the first 6; bend: alpha[4]; spring: rest length),
 * global_idx [n] (compact row of the element's first row).                    */
int admm_hip_read_rest(admm_hip_ctx *ctx, int batch, double *weight, double *rest, int32_t *global_idx);

/* one local step on caller-supplied positions (no global step): runs the batch
 * kernels on x_cur = x and returns; used by the per-project parity tests.     */
int admm_hip_local_step_only(admm_hip_ctx *ctx, const double *x_cur);
/* the assembled right-hand side b = M x_bar + dt^2 D^T W^2 (z - u) as the last local step left it on the device, y [n_nodes][3] in
 * the caller's node order.  admm_hip_local_step_only ends with the assembly and runs no solve, so local_step_only + debug_rhs observes
 * exactly what the sweeps would be handed (M x_bar: of the last admm_hip_step's prologue).  In a sharded context: this rank's vector
 * before any all-reduce (the ranks' vectors sum to b).  Parity tests only; no product path calls it.                              */
int admm_hip_debug_rhs(admm_hip_ctx *ctx, double *y);
/* one project() of every local element of `batch` on caller-supplied D_i x rows
 * (element-major [n_local][rows]) instead of the gather: replays the per-project
 * golden tuples captured from the reference (tests/golden/project_*.npz).       */
int admm_hip_local_step_dx(admm_hip_ctx *ctx, int batch, const double *dx);
/* solves A X = B for B = [n_nodes][3] on the device factor (parity tests).    */
int admm_hip_solve_only(admm_hip_ctx *ctx, const double *b, double *x);
/* host-side product with the assembled scalar matrix: y = A_s * x, x,y [n][3] */
int admm_hip_apply_A(admm_hip_ctx *ctx, const double *x, double *y);
/* CPU evaluation of the factor's two panel sweeps -- validation hook for the
 * CPU test-suite only; no product path calls it.                               */
int admm_hip_debug_panel_solve_host(admm_hip_ctx *ctx, const double *b, double *x);

/* One function of the per-lane math (csrc/local_math.hpp) as the DEVICE build of the header executes it, on n records
 * (parity tests: tests/test_gpu_parity.py, tests/test_device_math.py compare every bit).  in / out hold n records,
 * element-major; doubles per record, in -> out:
 *   op 0 admm_log 1 -> 1      op 1 admm_exp 1 -> 1       (glibc's algorithms restated; against the host's libm)
 *   op 2 sqrt_in_1_4 1 -> 1   op 3 sqrt_ge_1 1 -> 1      op 4 rcp_in_1_2 1 -> 1      op 5 eig_hypot 2 -> 1
 *   op 6 svd3 9 -> 21         op 7 oriented_svd 9 -> 21  (U, s0 s1 s2, V; matrices column-major: m00 m10 m20 m01 ...)
 *   op 8 svd32 6 -> 12        (U's first two columns, s0 s1, V 2x2; all column-major)
 *   op 9 mt_cstep 12 -> 9     ([stx fx dx sty fy dy stp fp dp stpmin stpmax brackt] -> [stx fx dx sty fy dy stp brackt info])
 * The hook guarantees: one lane per record; workgroups of 256 threads, so record i runs on lane i % 64 of wave i / 64;
 * lanes beyond n return before any of the function's code; op is a kernel argument (wave-uniform), a launch runs one
 * function.  A caller can therefore compose the waves that mt_cstep's wave-uniform branches see.  n <= 2^30.          */
int admm_hip_debug_math(admm_hip_ctx *ctx, int op, int64_t n, const double *in, double *out);
/* Unit-test hooks for the kernels of the device factorization (csrc/factor_dev.hpp), host arrays in and out, column-major:
 *  gemm:      C (m x n, ldc) = beta C + alpha opA(A) opB(B) through gemm_f64_kernel; flags: 1 A transposed (stored k x m), 2 B transposed
 *             (stored n x k), 4 only tiles on / below the diagonal, 8 sum from the tile's first column, 16 from max(tile row, tile column);
 *             size_a / size_b / size_c: doubles in the arrays.
 *  potrf_inv: blk (w x w, ld, w <= 64; lower triangle read) <- its Cholesky factor, out (w x w, ld) <- the factor's inverse;
 *             returns ADMM_ERR_FACTOR when a pivot is not positive.                                                              */
int admm_hip_debug_gemm(admm_hip_ctx *ctx, int m, int n, int k, int lda, int ldb, int ldc, int flags, double alpha, double beta,
                        const double *A, int64_t size_a, const double *B, int64_t size_b, double *C, int64_t size_c);
int admm_hip_debug_potrf_inv(admm_hip_ctx *ctx, int w, int ld, double *blk, double *out);
/* launch mode of the last admm_hip_step (tests: "was the multi-GPU iteration really replayed as a graph?"):
 * *iter_graph = 1 when a per-iteration HIP graph exists, *frame_graph = ADMM iterations of the whole-frame graph (0: none),
 * *graph_launches = graph launches issued by the context so far.  Any pointer may be NULL.                               */
int admm_hip_debug_graph_state(admm_hip_ctx *ctx, int *iter_graph, int *frame_graph, int64_t *graph_launches);
/* which kernels the collision batches launch for the current shape list: 0 the frictionless ones, 1 the friction form, 2 its moving form,
 * 3 the framed form, 4 the shell form (a list that names an open mesh), 5 the self-collision form (a list that names a sheet surface that
 * collides with itself).  A call that changes the value drops the captured graphs.                                                       */
int admm_hip_debug_collision_form(admm_hip_ctx *ctx, int *form);

typedef struct admm_hip_info {
    int64_t n_nodes, n_elems_total, n_elems_local, rows_compact;
    int64_t nnz_A;            /* scalar n x n system, lower triangle          */
    int64_t nnz_L;            /* entries of the supernodal factor panels read per triangular sweep */
    int64_t panel_bytes;      /* device bytes of the factor panels            */
    int64_t n_supernodes, n_levels, max_super_cols, max_super_rows;
    int64_t solve_contrib_rows; /* sum of below-diagonal block rows            */
    double  t_order_s, t_symbolic_s, t_numeric_s, t_upload_s; /* finalize phases */
    int32_t rank, world, device_id, host_threads;
    int32_t dense_solve;      /* 1: small system, solved as x = A_s^-1 b with the explicit inverse (see admm_hip_finalize) */
    int32_t device_factor;    /* 1: the numeric factorization ran on the GPU (csrc/factor_dev.hpp), 0: on the host */
    int64_t rhs_slots;        /* 24-byte slots the local kernels write and the RHS gather reads per ADMM iteration (this rank) */
    /* sharding: what THIS rank's sweeps stream and what it exchanges (one rank / contiguous shards: own = the whole factor, top = 0).
     * Entries are counted like nnz_L: k(k+1)/2 + r k per supernode.                                                          */
    int64_t sweep_entries_own;      /* supernodes of this rank's own subtrees (both sweeps)                                  */
    int64_t sweep_entries_top;      /* the replicated top of the tree (forward sweep: all of it, on every rank)              */
    int64_t sweep_entries_top_bwd;  /* the part of the top this rank's backward sweep covers (separators it reads + ancestors) */
    int64_t nodes_own, nodes_top;   /* nodes of the own subtrees / of the replicated top                                     */
    int64_t comm_doubles_iter;      /* doubles summed across the ranks per ADMM iteration (one collective; two with dist_top) */
    int64_t comm_doubles_frame;     /* additionally once per frame (subtree shards: the full x before the velocity update)   */
    /* rank-local factorization (subtree shards, admm_hip_set_factor_local): what THIS rank factors and keeps on its device   */
    int64_t factor_doubles_resident; /* doubles of factor panels (+ root inverses) resident on this rank's device; one rank / contiguous shards /
                                        factor_local = 0: the whole factor = panel_bytes / 8                                     */
    int64_t front_doubles;           /* doubles of frontal matrices this rank's numeric factorization held at once (0: factored on the host) */
    int64_t factor_exchange_doubles; /* doubles summed across the ranks ONCE per factorization (the subtree roots' update matrices) */
    int32_t factor_local;            /* 1: this rank factored only its own subtrees + the replicated top                          */
    int32_t dist_top;                /* 1: distributed top -- the top of the tree is ONE root supernode whose product with its explicit inverse is split
                                        by rows across the ranks (subtree shards of 2 / 4 / 8 / 16 ranks; ADMM_HIP_DIST_TOP=0: replicated top): two small
                                        collectives per ADMM iteration instead of one, no replicated sweep                                         */
} admm_hip_info;
int admm_hip_get_info(admm_hip_ctx *ctx, admm_hip_info *info);
/* Rank-local factorization (default on; ADMM_HIP_FACTOR_LOCAL=0 / 1 overrides).  Under subtree sharding with world > 1 a rank sweeps
 * only its own subtrees and the replicated top of the elimination tree, so that is all it assembles, factors and keeps on its device:
 * System::initialize's ONE solver.compute(A) (System.cpp:138-140) is split N ways instead of repeated N times.  The update matrices
 * of the subtree roots meet in ONE all-reduce through the installed transport (owner's values + zeros elsewhere), after which every
 * rank factors the top from the same bits.  That makes admm_hip_finalize and admm_hip_recompute_weights COLLECTIVE calls in this
 * mode: the transport must be installed before finalize and every rank must be inside the call at the same time.  With no transport
 * installed at finalize (or on = 0, or contiguous shards) every rank factors the whole matrix as before.  Before finalize only.  */
int admm_hip_set_factor_local(admm_hip_ctx *ctx, int on);

/* per-phase device timing of the last admm_hip_step (HIP events on the
 * context's stream; enabled with admm_hip_enable_timing).  ms per frame.      */
typedef struct admm_hip_timing {
    float prologue_ms, local_ms, rhs_ms, allreduce_ms, solve_fwd_ms, solve_bwd_ms, epilogue_ms, total_ms;
    int32_t iters;
} admm_hip_timing;
/* on = 1: events around the phases of every ADMM iteration (eager launches); on = k > 1: around every k-th iteration only
 * -- a HIP event is a barrier packet that costs ~5 us of launch overlap -- the other iterations run event-free (one graph
 * replay each where a graph exists) and the phase sums are scaled to the frame; total_ms is always the real span.      */
int admm_hip_enable_timing(admm_hip_ctx *ctx, int on);
int admm_hip_get_timing(admm_hip_ctx *ctx, admm_hip_timing *t);
/* the step BEFORE the last one (each timed step keeps its events until the step after the next is recorded): read it after the next
 * step has been queued and the GPU never waits for the host between frames.  ADMM_ERR_STATE if it was not timed / already read. */
int admm_hip_get_timing_previous(admm_hip_ctx *ctx, admm_hip_timing *t);

/* ---- residuals and convergence-based early exit ------------------------------------------
 * The reference only DESCRIBES these (comment at System.cpp:64-65, paper Eq. 22-23):
 *     r = W (Dx - z)            primal residual, with the Dx the local step used
 *     s = D^T W^T W (z - z_prev) dual residual
 * With tracking on, every ADMM iteration of admm_hip_step also computes |r|_2 and |s|_2 (extra
 * work inside the tet / anchor kernels plus one more gather: about +9 % per iteration at 1M tets; off by default = the reference's loop).
 * admm_hip_get_residuals copies the norms of the last step; *n_iters = ADMM iterations that step ran.
 * admm_hip_set_tolerance(eps_r, eps_s, check_every): with eps_r > 0 the ADMM loop of a step ends as
 * soon as |r| <= eps_r and |s| <= eps_s, tested every `check_every` iterations (each test is one
 * host-device round trip); admm_iters stays the upper bound.  Tracking is switched on implicitly. */
int admm_hip_enable_residuals(admm_hip_ctx *ctx, int on);
int admm_hip_get_residuals(admm_hip_ctx *ctx, double *r_norm, double *s_norm, int capacity, int *n_iters);
int admm_hip_set_tolerance(admm_hip_ctx *ctx, double eps_r, double eps_s, int check_every);

/* ---- energies and the per-iteration ADMM objective ---------------------------------------------------------------------------------
 * Extension, no reference counterpart (the reference never evaluates what it minimises).  Every frame the solver minimises the incremental
 * potential of the paper,   Phi(x) = 1 / (2 dt^2) |x - x_bar|^2_M + sum_i E_i(D_i x),   with d = D_i x the element's compact rows exactly
 * as the local step forms them (the scaled dual variable u plays no part) and s the element's scale:
 *   TET_NH      s [mu/2 (I1 - L - 3) + lambda/8 L^2],  I1 = |d|^2_F, J = det d, L = log(J J); +inf when J <= 0 or not finite      s = rest volume
 *   TET_STVK    s [mu |E|^2_F + lambda/2 tr^2 E],  E = (d^T d - I) / 2; finite for inverted elements too                          s = rest volume
 *   TRI_FUNG    s mu/2 (exp(I1 - 3) - 1),  I1 = |d|^2_F + 1/g, g = det(d^T d); +inf when g <= 0 or the exponential overflows      s = rest area
 *   TET_LINEAR, TET_VOLUME, TRI_STRAIN, TRI_AREA   s/2 |d - p|^2, p the kind's projection of d (TRI_STRAIN: U(:, :2) V^T; its strain
 *               limits are a hard clamp and carry no energy)                                                  s = stiffness * rest measure
 *   SPRING      s/2 |d - L d / |d||^2 (p = 0 where |d| <= 0);   BEND   s/2 |d - p|^2, p the hinge projection                     s = stiffness
 *   ANCHOR      active: w^2/2 |x - t|^2, released: 0.  A hard constraint in z, zero at convergence: reported as `anchor`, never part of
 *               `elastic`.                                                                                    s = weight^2
 *   COLLISION, GENERIC   not evaluated: the value is 0 and the batch is counted in batches_skipped.
 * One definition, csrc/energy.hpp, compiled without fused multiply-adds for the host and the device: both give the same bits.  An element
 * whose energy is not finite adds nothing to a sum and is counted instead (n_infinite).  Sums use no atomics and a fixed order that depends
 * only on the element (node) count (csrc/kernels_energy.hpp documents it): two calls on the same state return the same bits, whatever
 * ADMM_HIP_TPB, ADMM_HIP_LOCAL_MULTI and ADMM_HIP_PRERED are.  The node terms are summed in the caller's node order.
 * Every call below reads the device state as it stands (after finalize, between frames), runs on the context's stream and waits for it;
 * none writes x, v, u, z, the warm starts, the cost counters or the sides, and none drops a captured graph.  Their buffers are created by
 * the first call that needs them; a context that never calls them launches exactly what it did.  Cost: not measured.
 *   admm_hip_energy          kinetic = 1/2 sum m v^2,  gravity = -sum m g x over every ADMM_EXPLICIT_CONST entry and its nodes (wind has no
 *                           potential and is left out),  elastic = the evaluated batches' totals except the anchors', added in batch
 *                           order,  anchor = the anchor batches' totals,  n_infinite, batches_skipped.
 *   admm_hip_batch_energy    one batch: its total, per_elem [n_local] in the order of admm_hip_read_local, the count of non-finite
 *                           elements.  Any pointer may be NULL.  A batch that is not evaluated: zeros.
 *   admm_hip_batch_energy_dx a parity entry like admm_hip_local_step_dx: the same kernel on caller-supplied rows dx [n_local][rows].
 *                           ADMM_ERR_UNSUPPORTED for a batch that is not evaluated.
 *   admm_hip_read_energy_scale  s [n_local] of this rank's elements (an anchor's: the weight^2 of admm_hip_set_weights as it stands).
 *   admm_hip_energy_query    context-free host evaluation, the device's bits; needs no GPU: dx [n][rows], params [n][ADMM_KIND_PARAMS],
 *                           rest [n][12] as admm_hip_read_rest lays it out (read for springs and hinges only; an anchor's target in
 *                           rest[0..2], active = params[1] != 0), scale [n] -> energy [n].  ADMM_ERR_ARG: a kind that is not evaluated,
 *                           n < 0, a NULL array with n > 0.  n = 0: ADMM_OK, nothing is read.
 *   admm_hip_enable_objective  on != 0: every ADMM iteration of admm_hip_step appends, after its global step, inertia(x_k) =
 *                           1 / (2 dt^2) sum m (x_k - x_bar)^2 (x_bar from the prologue's M x_bar) and elastic(x_k); the objective is their
 *                           sum.  The loop then runs eagerly, as under residual tracking; x and v are bitwise what they are with it off.
 *                           ADMM_ERR_UNSUPPORTED in a sharded context (world > 1): under subtree shards the full x exists only at the
 *                           end of the frame.
 *   admm_hip_get_objective   the two histories of the last step, at most `capacity` entries; *n_iters = the iterations it recorded (an
 *                           early exit ends the history where the loop ends: the length of admm_hip_get_residuals').
 * Sharded contexts: elastic, anchor, the counts and admm_hip_batch_energy cover THIS rank's local elements (admm_hip_local_elements); the
 * ranks' values add up to the one-rank value.  The node terms cover all nodes and are the same, bit for bit, on every rank.           */
typedef struct admm_hip_energy_totals {
    double kinetic, gravity, elastic, anchor;
    int64_t n_infinite, batches_skipped;
} admm_hip_energy_totals;
int admm_hip_energy(admm_hip_ctx *ctx, admm_hip_energy_totals *out);
int admm_hip_batch_energy(admm_hip_ctx *ctx, int batch, double *total, double *per_elem, int64_t *n_infinite);
int admm_hip_batch_energy_dx(admm_hip_ctx *ctx, int batch, const double *dx, double *per_elem);
int admm_hip_read_energy_scale(admm_hip_ctx *ctx, int batch, double *s);
int admm_hip_energy_query(int kind, int64_t n, const double *dx, const double *params, const double *rest, const double *scale, double *energy);
int admm_hip_enable_objective(admm_hip_ctx *ctx, int on);
int admm_hip_get_objective(admm_hip_ctx *ctx, double *inertia, double *elastic, int capacity, int *n_iters);

/* ---- elastic forces and tet stresses: the gradient of the energies above ---------------------------------------------------------------
 * Extension, no reference counterpart.  g = dE_i/dd in the element's compact rows (the layout of d: 9 / 6 / 3 rows), the nodal internal
 * force f = -sum_i D_i^T g_i, and the tets' Cauchy stress.  One definition, csrc/gradient.hpp, compiled without fused multiply-adds for the
 * host and the device: both give the same bits.
 *   Exact derivatives of the energy:  TET_NH  s [mu d + (lambda L / 2 - mu) cof(d) / J];  TET_STVK  s d (2 mu E + lambda tr(E) I);
 *     TRI_FUNG by the chain rule through I1;  SPRING, BEND, ANCHOR  s (d - p) (an anchor: w^2 (x - t), released: 0);  TET_LINEAR,
 *     TRI_STRAIN  s (d - p), p the nearest rotation / isometry.
 *   PROJECTIVE FORCE ONLY:  TET_VOLUME, TRI_AREA return s (d - p) with the kind's projection p.  That is the force projective dynamics
 *     applies, NOT the derivative of the stored energy: the projections stop after 4 / `iters` Newton steps, and finite differences of
 *     the energy differ from it by 2 % to 90 % where the limits are active (both are exactly 0 where they are not).
 *   Not finite: where the energy is not finite (TET_NH at J <= 0, TRI_FUNG at g <= 0) or an entry overflows, every entry of the element's
 *     g is NaN; the element adds zeros to every corner force and node sum and is counted in n_nonfinite.
 *   Stress (TET_* only): Cauchy sigma = (g d^T) / (V J), V the rest volume, off-diagonal pairs symmetrised as (a + b) / 2; seven doubles per
 *     tet: xx, yy, zz, xy, xz, yz, von Mises.  All seven are NaN where J <= 0.
 * Every compute call reads the device state as it stands, runs on the context's stream and waits for it; none writes x, v, u, z, the warm
 * starts, the cost counters or the sides, and none drops a captured graph.  Their buffers are created by the first call that needs them;
 * a context that never calls them uploads and launches exactly what it did.  Sums use no atomics and a fixed order (csrc/
 * kernels_gradient.hpp): a node adds its incident corners by a compensated sequential sum (the exact sum rounded once, to second order in
 * 2^-53) in batch order, then local element order, then the element's corners as the caller listed them -- whatever the elimination order, ADMM_HIP_TPB, ADMM_HIP_LOCAL_MULTI and ADMM_HIP_PRERED are.  Cost: not
 * measured.
 *   admm_hip_batch_gradient     one batch: g [n_local][rows] and corner_forces [n_local][nodes][3] (-D_i^T g, the corners as the caller
 *                              listed them), element-major in the order of admm_hip_read_local, and the count of elements whose g is not
 *                              finite.  Any pointer may be NULL.  A batch that is not evaluated (COLLISION, GENERIC): zeros.
 *   admm_hip_batch_gradient_dx  a parity entry like admm_hip_batch_energy_dx: the same kernel on caller-supplied rows dx [n_local][rows]
 *                              -> g.  ADMM_ERR_UNSUPPORTED for a batch that is not evaluated.
 *   admm_hip_batch_stress       stress7 [n_local][7] of a tet batch and the count of tets whose stress is not finite.
 *                              ADMM_ERR_UNSUPPORTED for a batch that is not a tet batch.
 *   admm_hip_node_forces        f_elastic, f_anchor [n_nodes][3] in the caller's node order (either may be NULL): the internal forces of
 *                              the evaluated batches except the anchors', and of the anchor batches.  info (may be NULL): n_nonfinite
 *                              over all evaluated batches, batches_skipped (COLLISION, GENERIC).  A node with no element: exactly 0.
 *   admm_hip_gradient_query     context-free host evaluation, the device's bits; needs no GPU: the arguments of admm_hip_energy_query
 *                              -> g [n][rows]; the same argument checks.
 *   admm_hip_stress_query       likewise for the tet kinds: dx [n][9], params [n][ADMM_KIND_PARAMS], volume [n] (the rest volumes; the
 *                              scale s follows from them as in admm_hip_read_energy_scale) -> stress7 [n][7].  ADMM_ERR_ARG: a kind that
 *                              is not a tet kind, n < 0, a NULL array with n > 0.  n = 0: ADMM_OK, nothing is read.
 * Sharded contexts: every call covers THIS rank's local elements (admm_hip_local_elements); the ranks' node vectors add up to the
 * one-rank vector within 2^-52 sum |share| per component (they are not gathered into one).                                                                                    */
typedef struct admm_hip_force_info {
    int64_t n_nonfinite, batches_skipped;
} admm_hip_force_info;
int admm_hip_batch_gradient(admm_hip_ctx *ctx, int batch, double *g, double *corner_forces, int64_t *n_nonfinite);
int admm_hip_batch_gradient_dx(admm_hip_ctx *ctx, int batch, const double *dx, double *g);
int admm_hip_batch_stress(admm_hip_ctx *ctx, int batch, double *stress7, int64_t *n_nonfinite);
int admm_hip_node_forces(admm_hip_ctx *ctx, double *f_elastic, double *f_anchor, admm_hip_force_info *info);
int admm_hip_gradient_query(int kind, int64_t n, const double *dx, const double *params, const double *rest, const double *scale, double *g);
int admm_hip_stress_query(int kind, int64_t n, const double *dx, const double *params, const double *volume, double *stress7);

/* ---- Anderson acceleration of the ADMM iteration ---------------------------------------------------------------------------------------
 * Extension, no reference counterpart (Zhang, Peng, Ouyang, Deng: Accelerating ADMM for Efficient Simulation and Optimization, 2019).
 * One ADMM iteration maps the state s = (z, u) over all elements of all built-in batches to G(s): the right-hand side and the solve turn
 * s into x, the local step turns (x, u) into the next (z, u).  With a window m >= 1 every iteration of admm_hip_step runs, between its
 * local step and its right-hand side,
 *     g = G(s_in) (what the local step left),  f = g - s_in (s_in: the z, u the iteration started from; at a frame's first iteration
 *     z = D x),  rho = sum_e w_e^2 (|dz_e|^2 + |du_e|^2)   (its u part is the square of the primal residual of admm_hip_get_residuals).
 *   Accept  -- the frame's first iteration, the first one after a reset, or rho < the rho of the last accepted iteration: s_def <- g;
 *     (g, f) joins the history (the last m + 1 entries); with m_k = entries - 1 differences dF, dG of adjacent entries, theta solves
 *     (dF^T W^2 dF + 1e-12 tr(dF^T W^2 dF) / m_k I) theta = dF^T W^2 f and s_out = g - sum_j theta_j dG_j (m_k = 0: s_out = g).
 *   Reset   -- otherwise: s_out <- s_def, the history is emptied, the next iteration is accepted whatever its rho.
 *   The LAST scheduled iteration of a step never extrapolates (s_out = g, or s_def on a reset): what ends a frame and what carries u into
 *     the next frame or a checkpoint is an un-extrapolated output of G.  A tolerance exit (admm_hip_set_tolerance) is decided on the host
 *     one iteration later and may end the frame on an extrapolated iterate.
 * s_out goes to the batches' z and u (and the right-hand-side shares are rebuilt from it) before the iteration goes on.  The history
 * lives within a frame: a checkpoint holds what it held.  The hyperelastic kinds' warm start is not part of s; the safeguard covers
 * that.  The tracked residuals and the tolerance test keep their definitions, against the iterate that entered the iteration.
 * Everything is decided on the device: no host synchronisation is added.  Sums use no atomics and an order that depends only on the
 * element counts: results are bitwise reproducible.  One definition of the small solve, csrc/anderson.hpp, for host and device.
 * Cost: the history is 2 (m + 1) copies of (z, u), allocated by the first step that needs it (1M-tet bar, m = 6: 2.0 GB); a
 * step with m >= 1 runs the eager loop (no captured graph, like residual tracking) and stores the tets' z (admm_hip_keep_z is moot).
 *   admm_hip_set_acceleration   window m, 0 <= m <= 8 (else ADMM_ERR_ARG); 0 = off, the default: admm_hip_step launches exactly what it
 *                              did, and captured graphs stay valid.  Before or after finalize, on a host-only context too.  With
 *                              m >= 1 admm_hip_step returns ADMM_ERR_UNSUPPORTED for a context with user-defined (generic) batches
 *                              or a sharded one (world > 1: the Gram matrix would have to be all-reduced).
 *   admm_hip_get_acceleration_log  one record per ADMM iteration of the last step, at most `capacity`; *n = the iterations it ran.
 *                              gram, rhs: the m_used x m_used system the device solved before regularisation (row stride 8; differences
 *                              oldest first); theta: its solution (zeros when solve_failed: a pivot was not positive; no extrapolation
 *                              then); on a reset m_used = 0.  extrapolated: s_out differs from g by the theta combination.
 *   admm_hip_get_acceleration_default  the stored s_def of one batch, z and u [n_local][rows] in the layout of admm_hip_read_local
 *                              (either may be NULL).  ADMM_ERR_STATE before the first accelerated step.
 *   admm_hip_acceleration_query  context-free host twin of the device's solve, the same bits; needs no GPU: gram [m_k][m_k] row-major
 *                              (its lower triangle is read), rhs [m_k] -> theta [m_k] (zeros where a pivot is not positive).
 *                              ADMM_ERR_ARG: m_k outside 1..8, a NULL array.                                                          */
typedef struct admm_hip_acceleration_record {
    double rho;
    int32_t accepted, m_used, extrapolated, solve_failed;
    double theta[8], gram[64], rhs[8];
} admm_hip_acceleration_record;
int admm_hip_set_acceleration(admm_hip_ctx *ctx, int window);
int admm_hip_get_acceleration_log(admm_hip_ctx *ctx, admm_hip_acceleration_record *records, int capacity, int *n);
int admm_hip_get_acceleration_default(admm_hip_ctx *ctx, int batch, double *z, double *u);
int admm_hip_acceleration_query(int m_k, const double *gram, const double *rhs, double *theta);

/* ---- contact and anchor reactions: which nodes touch something, and how hard -----------------------------------------------------------
 * Extension, no reference counterpart.  A frame's last global solve satisfies
 *     M (x - x_bar) / dt^2 = sum_i D_i^T w_i^2 (z_i - u_i - D_i x)        (up to the linear solve's residual)
 * with z_i, u_i what the last local step stored and x the final position.  For the two kinds with D_i = I on one node, COLLISION and
 * ANCHOR, element i's term is the force the constraint exerted on its node in that frame:
 *     f_i = w_i^2 ((z_i - u_i) - x_node)        depth_i = |u_i| = sqrt((u0 u0 + u1 u1) + u2 u2)        point_i = z_i
 * and a node is IN CONTACT where depth > depth_min.  A free node is not at u = 0 exactly -- u + (dx - (dx + u)) leaves rounding residue of
 * a few ulp of |x| -- so depth_min is the caller's, in length units, >= 0 (ADMM_ERR_ARG otherwise, NaN included): choose it above that
 * residue and below any penetration you care about.  One definition, csrc/reaction.hpp, compiled without fused multiply-adds for the host
 * and the device: both give the same bits.  w^2 is the weight^2 the batch holds (admm_hip_set_weights / admm_hip_recompute_weights).
 * Every compute call reads the device state as it stands, runs on the context's stream and waits for it once; none writes x, v, u, z, the
 * warm starts, the cost counters or the sides, and none drops a captured graph.  Their buffers are created by the first call; a context
 * that never calls them uploads and launches exactly what it did.  No atomics, fixed orders (csrc/kernels_reaction.hpp): a node adds its
 * elements sequentially in batch order, then local element order; its depth is the largest of its collision elements' and its point the
 * z of that element (ties: the first); the contacts come in ascending node index; the resultant is summed in the order csrc/reaction.hpp
 * states.  Two calls on the same state return the same bits.  Cost: not measured.
 * Order of the checks: the call's own arguments (ADMM_ERR_ARG; a batch of another kind: ADMM_ERR_UNSUPPORTED), then a host-only context
 * (device_id < 0: ADMM_ERR_HIP, like every compute call), then ADMM_ERR_STATE before finalize, with no usable factor, or before the first
 * admm_hip_step: a reaction is that of the last frame.
 * Valid until the state is next changed from outside: the entries combine the u and z of the last admm_hip_step with the x the device
 * holds now, and the library does not notice admm_hip_set_x / admm_hip_upload_state, admm_hip_write_local, admm_hip_set_weights or a
 * local_step_only / local_step_dx in between -- after any of them the values mean nothing until the next admm_hip_step.
 *   admm_hip_batch_reaction     one COLLISION or ANCHOR batch: f [n_local][3] and depth [n_local] in the order of admm_hip_read_local.
 *   admm_hip_node_reactions     f_contact, f_anchor [n_nodes][3] in the caller's node order: the collision batches' and the anchor batches'
 *                              sums.  info: the batches reported (batches_collision, batches_anchor) and passed over (batches_skipped: every
 *                              other kind), n_contacts = the nodes with depth > 0.  A node with no such element: exactly 0.
 *   admm_hip_get_contacts       the nodes with depth > depth_min as records {node, f, point, depth}, ascending node index; f = the node's
 *                              f_contact.  *count = how many there are; records [capacity] receives the first min(count, capacity).
 *                              The price of the one synchronisation: the count is not known when the copy is queued, so the call
 *                              moves min(capacity, n_nodes) records of 64 bytes from the device whatever the count is (only the filled
 *                              ones reach `records`).  A caller with few contacts among many nodes passes a small capacity and calls
 *                              again when *count exceeds it, or takes the count from admm_hip_contact_resultant first.
 *   admm_hip_contact_resultant  out6 = {sum f, sum (point - pivot) x f} over those contacts (pivot NULL: the origin), *count likewise.
 *   admm_hip_reaction_query     context-free host evaluation, the device's bits; needs no GPU: w2 [n], u, z, x [n][3] -> f [n][3],
 *                              depth [n], flag [n] (depth > depth_min), resultant6 over the flagged elements in index order with
 *                              point = z.  ADMM_ERR_ARG: n < 0, depth_min not >= 0, a NULL input with n > 0.
 * Any output pointer may be NULL.
 * What it holds under the solver's options:
 *   every collision form (admm_hip_debug_collision_form 0-8): the report reads only u, z and x, which every form leaves by the same
 *     epilogue.  Friction's tangential part is inside f; contact attribution (below) tells normal and tangential parts apart.
 *   admm_hip_keep_z(ctx, 0): only the tet kernels honour it; the collision and anchor kernels store z in every iteration.
 *   an early exit by tolerance: the identity holds for the last iteration that ran.
 *   Anderson acceleration: every iteration writes its s_out to the batches' z and u and rebuilds the right-hand-side shares from them
 *     before the solve, so what the batches hold after a frame is what the last solve consumed, extrapolated or not, reset or not.
 *   a released anchor (active = 0) goes through the same formula, no special case: its z is x_prev + u with x_prev the iterate the last
 *     local step saw, so f = w^2 (x_prev - x) up to rounding residue -- the last iteration's increment, zero at convergence.  The same holds
 *     for a collision element that touches nothing: its depth is residue (no contact), its f that increment.
 * Reactions on the triangles of a body or sheet surface: two-way contact, further below (admm_hip_set_surface_reaction), for the nodes
 * of other bodies; a self-contact's push stays one-sided.  Not covered: user-defined (GENERIC) batches, a
 * per-iteration history, a normal from more than the last mover (contact attribution, below, records the last one).
 * Sharded contexts: every call covers THIS rank's local elements; the ranks' node vectors add up to the one-rank vector (they are not
 * gathered into one), and a node's contact is reported by the rank that owns its collision element.                                    */
typedef struct admm_hip_reaction_info {
    int64_t batches_collision, batches_anchor, batches_skipped, n_contacts;
} admm_hip_reaction_info;
typedef struct admm_hip_contact {
    int32_t node;
    double f[3], point[3], depth;
} admm_hip_contact;
int admm_hip_batch_reaction(admm_hip_ctx *ctx, int batch, double *f, double *depth);
int admm_hip_node_reactions(admm_hip_ctx *ctx, double *f_contact, double *f_anchor, admm_hip_reaction_info *info);
int admm_hip_get_contacts(admm_hip_ctx *ctx, double depth_min, admm_hip_contact *records, int64_t capacity, int64_t *count);
int admm_hip_contact_resultant(admm_hip_ctx *ctx, double depth_min, const double pivot[3], double out6[6], int64_t *count);
int admm_hip_reaction_query(int64_t n, const double *w2, const double *u, const double *z, const double *x, double depth_min, const double *pivot,
                            double *f, double *depth, int32_t *flag, double *resultant6);

/* ---- contact attribution: WHAT a node touches -- owner entry, normal, normal / tangential parts, per-obstacle resultants -------------------
 * Extension, no reference counterpart; off unless asked for: a context that never enables it uploads and launches exactly what it did and
 * produces the same bits.  One definition, csrc/attribution.hpp, compiled without fused multiply-adds for the host and the device.
 * An entry q of the collision list MOVED an element's candidate when a coordinate's BITS differ between the point before the entry's
 * rule and the point behind the rule and before friction; an entry that is skipped or whose rule does not fire moved nothing.
 *     owner    the index of the last entry in list order that moved the candidate in that local step; -1: none did
 *     normal   of that last mover: d = after - before, len = sqrt((d0 d0 + d1 d1) + d2 d2), n = d / len; owner -1: exactly 0.  The
 *              direction of the push: a floor's normal, a sphere's radial, a closed mesh's outward direction at the closest point, for a
 *              node mirrored back by side memory or body self-collision the remembered / outer side
 *     split    of a reaction f about n: fn = (f0 n0 + f1 n1) + f2 n2, ft_j = f_j - fn n_j
 *   admm_hip_enable_contact_attribution  on != 0: every collision batch launches form 8 of the collision kernel (admm_hip_debug_collision_form
 *                              reads 8), whatever the list holds: everything form 7 knows -- z, u and the right-hand side keep the bits of
 *                              the form the list would otherwise select -- and one int32 owner and three doubles of normal stored per
 *                              collision element in EVERY local step, owner -1 with a zero normal included: what the record holds after a
 *                              frame is that of the last local step that ran, extrapolated by Anderson acceleration or not.  Callable
 *                              before or after finalize and between frames; the record is allocated by this call in a finalized context,
 *                              else by finalize, never by admm_hip_step; switching on fills it with owner -1, normal 0.  A change drops the
 *                              captured iteration and frame graphs, like a setter that changes the form; on = 0 returns the context to the
 *                              list's own form.  Allowed under sharding: each rank records its local elements.
 * The reports read the record; they check and behave like the reaction calls above (same order of checks, one synchronisation, buffers
 * created by the first call, no atomics, fixed orders, nothing written that a frame reads) and return ADMM_ERR_STATE while the switch is off.
 *   admm_hip_batch_contact_owner  one COLLISION batch (another kind: ADMM_ERR_UNSUPPORTED): entry [n_local] and normal [n_local][3] in the
 *                              order of admm_hip_read_local.
 *   admm_hip_get_contact_owners  the nodes and the order of admm_hip_get_contacts for that depth_min, as 64-byte records {node, entry,
 *                              normal, f_normal, f_tangent}: entry and normal are those of the collision element that gives the node its
 *                              depth and point (the largest depth, the first on ties), the split is of the node's f_contact.
 *   admm_hip_entry_resultants  out [(n_entries + 1)][6], count [n_entries + 1]: row q = {sum f, sum (point - pivot) x f} over the contacts
 *                              whose entry is q, in ascending node index, through exactly the two-stage sum of csrc/reaction.hpp; the
 *                              last row takes the contacts with entry -1 (deeper than depth_min from earlier iterations, moved by nothing
 *                              in the last local step).  n_entries must be the current list's length (ADMM_ERR_ARG otherwise).  The rows
 *                              add up to admm_hip_contact_resultant's up to the order of the additions.
 *   admm_hip_attribution_query  context-free host evaluation, the device's bits; needs no GPU: before, after, f [n][3] -> moved [n],
 *                              normal [n][3] (not moved: 0), fn [n], ft [n][3].  normal_in [n][3] (may be NULL): the split is about these
 *                              normals instead, and before / after may then both be NULL (moved 0, normal 0).  Outputs may be NULL.
 * Not covered: a normal from more than the last mover, a per-iteration history of owners.                                                   */
typedef struct admm_hip_contact_owner {
    int32_t node, entry;
    double normal[3], f_normal, f_tangent[3];
} admm_hip_contact_owner;
int admm_hip_enable_contact_attribution(admm_hip_ctx *ctx, int on);
int admm_hip_batch_contact_owner(admm_hip_ctx *ctx, int batch, int32_t *entry, double *normal);
int admm_hip_get_contact_owners(admm_hip_ctx *ctx, double depth_min, admm_hip_contact_owner *records, int64_t capacity, int64_t *count);
int admm_hip_entry_resultants(admm_hip_ctx *ctx, double depth_min, const double pivot[3], int n_entries, double *out, int64_t *count);
int admm_hip_attribution_query(int64_t n, const double *before, const double *after, const double *f, const double *normal_in, int32_t *moved, double *normal,
                               double *fn, double *ft);

/* ---- velocity damping per node group, applied after every frame ---------------------------------------------------------------------------
 * Extension, no reference counterpart.  A damping group is a range [node_first, node_first + node_count) of nodes in the caller's node
 * order with two rates in 1/s: drag >= 0 (ether drag) and internal >= 0 (the momentum-preserving damping of Mueller et al., Position
 * Based Dynamics, section 3.5: it removes the velocity that is not the group's rigid-body motion, so a thrown or spinning body keeps
 * flying and spinning while its jiggle dies).  Groups are disjoint.  admm_hip_step applies the filter to the v its epilogue left, with x
 * the new positions and m the nodes' scalar masses:
 *     M = sum m,  c = sum m x / M,  v_c = sum m v / M,  r = x - c
 *     L = sum m r x (v - v_c),  I = sum m (|r|^2 1 - r r^T),  omega = I^-1 L
 *     v <- v + beta ((v_c + omega x r) - v),  beta = internal dt / (1 + internal dt);    then v <- s v,  s = 1 / (1 + drag dt)
 * A group with internal == 0 takes v <- s v alone; a group with both rates zero is not touched.  A group of fewer than three nodes, or
 * with det I <= 1e-10 (tr I / 3)^3 (DAMPING_DEGENERATE: all nodes on a line), is degenerate: omega = 0, so its rotation is damped too.
 * One definition, csrc/damping.hpp, compiled without fused multiply-adds for the host and the device, with the sums' order written
 * out (64-node blocks from the group's first node, then the energies' two-stage reduction; no atomics): both give the same bits, which
 * depend neither on the elimination order nor on sharding.  Every rank of a sharded context filters its own whole copy of v.
 * Launches (csrc/kernels_damping.hpp), on the context's stream, eager, outside the captured graphs, inside the epilogue interval of the
 * timing events: five per frame when any group has internal > 0, one when only drag is set, none when every rate is zero or there is
 * no group -- such a context launches what it launched before and produces bitwise the same frames.
 *   admm_hip_add_damping_group   extension, no reference counterpart.  Before finalize only (ADMM_ERR_STATE after).  ADMM_ERR_ARG, with
 *                                admm_hip_last_error naming the value: a range outside the nodes added so far, node_count < 1, an overlap
 *                                with an earlier group (both are named), a negative or non-finite rate.  *group_id: 0, 1, ... in call order.
 *   admm_hip_set_damping         extension, no reference counterpart.  Before or after finalize: new rates for one group, in effect from the
 *                                next admm_hip_step on; no synchronisation, legal between steps on a caller's stream.
 *   admm_hip_get_group_moments   extension, no reference counterpart.  The sums above from the context's current x, v, computed on demand
 *                                (four launches, one synchronisation), also for a group with zero rates.  Needs a device and a finalized
 *                                context (ADMM_ERR_STATE otherwise).  t_total = sum 1/2 m |v|^2, t_rigid = 1/2 M |v_c|^2 + 1/2 omega . L;
 *                                inertia = xx yy zz xy xz yz about com; l about com.
 *   admm_hip_damping_query       extension, no reference counterpart.  Context-free host evaluation of one group of n nodes, the device's
 *                                bits; needs no GPU: m [n], x, v [n][3] -> v_out [n][3], *moments (of the input state).  Either output may
 *                                be NULL.  ADMM_ERR_ARG: n < 1, a NULL input, dt not > 0, a negative or non-finite rate.
 * Not covered: stiffness-proportional (Rayleigh) damping, per-element strain-rate damping, drag towards a wind field, groups that are
 * not ranges.                                                                                                                            */
typedef struct admm_hip_group_moments {
    double mass, com[3], p[3], l[3], inertia[6], omega[3], t_total, t_rigid;
    int64_t n_nodes;
    int32_t degenerate, pad_;
} admm_hip_group_moments;
int admm_hip_add_damping_group(admm_hip_ctx *ctx, int node_first, int node_count, double drag, double internal, int *group_id);
int admm_hip_set_damping(admm_hip_ctx *ctx, int group, double drag, double internal);
int admm_hip_get_group_moments(admm_hip_ctx *ctx, int group, admm_hip_group_moments *out);
int admm_hip_damping_query(int64_t n, const double *m, const double *x, const double *v, double dt, double drag, double internal,
                           double *v_out, admm_hip_group_moments *moments);

/* ---- pressure chambers: constant and gas-law surface loads, added before every frame -------------------------------------------------------
 * Extension, no reference counterpart.  A pressure chamber is an ordered list of oriented triangles tris [nt][3] over simulated nodes (the
 * caller's node ids) with a pressure law.  Once per frame, from the frame-start x, admm_hip_step works out the chamber's volume, area and
 * area vector with fixed-order sums, derives the pressure p and adds dt f_i / m_i to v:
 *     n_t = (x1 - x0) x (x2 - x0),   V = sum (r0 . (r1 x r2)) / 6,   A = sum |n_t| / 2,   N = sum n_t / 2       (r_k = x_k - o, o the
 *     f_i = p sum_{t with i} n_t / 6                                                        first triangle's first node: V loses no digits
 *                                                                                           to the chamber's distance from the origin)
 * For a closed chamber f_i is exactly p dV/dx_i and the forces add up to no net force and no net torque.  The normal of a triangle
 * follows its orientation: outward normals and p > 0 inflate.  Laws (params[2]):
 *   ADMM_PRESSURE_CONSTANT {p, unused}         p as given (gauge; negative: suction, or ambient pressure on a body with outward normals)
 *   ADMM_PRESSURE_GAS      {amount, ambient}   p = amount / V - ambient (isothermal).  A frame whose V is not > 0 or not finite gets
 *                                              p = 0 and adds one to the chamber's `collapsed` counter.
 * A constant chamber with p == 0, or a gas chamber with amount == 0 and ambient == 0, is inactive: it is passed over, and a node in no
 * active chamber is not written.  A node in two chambers (a septum) receives both.
 * Order in the frame: after the body surfaces' update and the side latch, before gravity, the constant accelerations and the wind --
 * pressure reads the frame-start surface the collision kernels see, and its increment is in v before gravity is added and before the
 * wind reads v.  One definition, csrc/pressure.hpp, compiled without fused multiply-adds for the host and the device, with the sums'
 * order written out (64-triangle blocks from the chamber's first triangle, then the energies' two-stage reduction; the per-node sum over
 * a node CSR ordered by chamber, triangle, corner; no atomics): both give the same bits, which depend neither on the elimination order
 * nor on sharding.  Every rank of a sharded context applies the load to its own whole copy of v.
 * Launches (csrc/kernels_pressure.hpp), on the context's stream, eager, outside the captured graphs, inside the prologue interval of the
 * timing events: three per frame when any chamber is active, none otherwise -- a context without chambers launches and uploads what it
 * did before and produces bitwise the same frames.
 *   admm_hip_add_pressure_chamber  extension, no reference counterpart.  Before finalize only (ADMM_ERR_STATE after).  ADMM_ERR_ARG, with
 *                                  admm_hip_last_error naming the value: nt < 1, a node id outside the nodes added so far, a triangle
 *                                  naming a node twice, an unknown mode, a non-finite parameter; in gas mode an edge that is not shared
 *                                  by exactly two oppositely oriented triangles (the edge is named).  *chamber: 0, 1, ... in call order.
 *                                  admm_hip_finalize refuses a gas chamber whose rest volume is not positive (chamber and volume named).
 *   admm_hip_set_pressure          extension, no reference counterpart.  Before or after finalize: a new law for one chamber, in effect from
 *                                  the next admm_hip_step on; no synchronisation, legal between steps on a caller's stream.  A change to
 *                                  gas mode checks closedness again.
 *   admm_hip_get_chamber_state     extension, no reference counterpart.  The record from the context's current x, computed on demand (two
 *                                  launches, one synchronisation), also for an inactive chamber; changes nothing.  `collapsed` is the
 *                                  frames counted so far.  Needs a device and a finalized context (ADMM_ERR_STATE otherwise).
 *   admm_hip_pressure_query        extension, no reference counterpart.  Context-free host evaluation, the device's bits; needs no GPU:
 *                                  x [nv][3], m [nv] (scalar masses), n_chambers chambers whose triangles are tris[tri_ptr[c] ..
 *                                  tri_ptr[c + 1]) (tri_ptr [n_chambers + 1], tris [..][3]), mode [n_chambers], params [n_chambers][2], dt
 *                                  -> dv [nv][3] (0 for a node in no active chamber), records [n_chambers] (collapsed: 1 if this
 *                                  evaluation collapsed).  Either output may be NULL.  ADMM_ERR_ARG: nv < 1, a NULL input, dt not > 0, an
 *                                  empty chamber, a node id out of range, an unknown mode, a non-finite parameter.
 * Not covered: no pressure term in admm_hip_energy or the objective, none in admm_hip_node_forces, no adiabatic exponent, no flow
 * between chambers; the load is explicit (frame-start geometry, one evaluation per frame).                                              */
enum { ADMM_PRESSURE_CONSTANT = 0, ADMM_PRESSURE_GAS = 1 };
typedef struct admm_hip_chamber_state {
    double volume, area, area_vector[3], pressure, resultant[3];      /* resultant = pressure * area_vector */
    int64_t n_tris, collapsed;
} admm_hip_chamber_state;
int admm_hip_add_pressure_chamber(admm_hip_ctx *ctx, int nt, const int32_t *tris, int mode, const double *params, int *chamber);
int admm_hip_set_pressure(admm_hip_ctx *ctx, int chamber, int mode, const double *params);
int admm_hip_get_chamber_state(admm_hip_ctx *ctx, int chamber, admm_hip_chamber_state *out);
int admm_hip_pressure_query(int64_t nv, const double *x, const double *m, int n_chambers, const int64_t *tri_ptr, const int32_t *tris,
                            const int32_t *mode, const double *params, double dt, double *dv, admm_hip_chamber_state *records);

/* ---- two-way contact: the reaction of a contact on the nodes of the body or sheet surface it landed on ------------------------------------
 * Extension, no reference counterpart; off unless asked for.  A node that lands on a body or sheet surface is pushed out; with a share
 * s_M > 0 on that surface M, the corners of the triangle it landed on receive -s_M times the node's reaction, as an impulse on v.
 * Once per frame, after admm_hip_step's epilogue and before the velocity damping, on the v the epilogue left:
 *   contacts   exactly the list of admm_hip_get_contacts(depth_min) (depth_min: admm_hip_set_surface_reaction_depth, default 0): K nodes,
 *              ascending caller's node index, f = the node's f_contact, point; entry = admm_hip_get_contact_owners' owner entry.
 *   status     the first that holds: ADMM_SURFACE_UNOWNED entry < 0; ADMM_SURFACE_OTHER the entry is no ADMM_SHAPE_MESH, or its mesh M is
 *              an obstacle, or s_M is 0; ADMM_SURFACE_SELF the node is one of M's own nodes (M's owner range: self-contacts of a
 *              self-colliding sheet or body do not react, the unbounded query would find the node's own 1-ring); else ADMM_SURFACE_REACTING.
 *   hit        point in the entry's coordinates as the collision rule takes it there (frame, then translation); M's closest point to it on
 *              the surface as this frame's start rebuilt it (the unbounded search, ties to the lowest triangle); lambda = the barycentric
 *              weights there; corners = the triangle's three vertices as nodes: what admm_hip_mesh_velocity_query returns as `weights`
 *              and `corner_ids` on a copy of the surface at the frame-start positions.
 *   shares     p = dt f once per contact; corner c of the hit adds (s_M lambda_c) p to its node.  Per destination node t, over its shares
 *              in ascending (contact index, corner): a = 0.0; a = a + share;  dv = a / m_t;  v_t = v_t - dv  (per component; every product
 *              rounded).  A node with no share is not touched.
 * One definition, csrc/surface_reaction.hpp, compiled without fused multiply-adds for the host and the device: both give the same bits.
 * Linear momentum: sum_t m_t dv_t = dt sum_k s_k f_k up to rounding (the weights add up to one).  Friction's tangential part is inside f
 * and reacts too.  The load is explicit: it has no term in admm_hip_energy or the objective, and it lags the push by one frame.  Angular
 * momentum is not exact: the force acts at the node, the reaction at the surface.
 * Launches (csrc/kernels_surface_reaction.hpp): the reaction and attribution reports' kernels, one kernel per contact for the hits, a
 * stable radix sort of the 3 K shares by destination (three launches per 8 bits of the node range) and one kernel that sums each node's
 * run in order -- no float atomics, no host synchronisation, K stays on the device; eager on the context's stream, outside the captured
 * graphs, inside the epilogue interval of the timing events.  Every buffer is allocated by the first admm_hip_set_surface_reaction with
 * share > 0 in a finalized context, or by finalize, never by admm_hip_step.  With all shares zero admm_hip_step launches and uploads
 * exactly what it did and produces bitwise the same frames.  The frame's launches overwrite the buffers of the reaction and attribution
 * reports (as a report for depth_min would).
 *   admm_hip_set_surface_reaction        share in [0, 1] for one body or sheet surface, in effect from the next admm_hip_step on; before or
 *                                        after finalize and between frames, no synchronisation.  Order of the checks: ADMM_ERR_ARG an
 *                                        unknown mesh, a mesh that is not a body or sheet surface, a share outside [0, 1] or NaN; then
 *                                        ADMM_ERR_STATE share > 0 while contact attribution is off; then ADMM_ERR_UNSUPPORTED share > 0 in a
 *                                        sharded context (a destination may live on another rank).  The other way round,
 *                                        admm_hip_enable_contact_attribution(ctx, 0) returns ADMM_ERR_STATE and admm_hip_set_shard with
 *                                        world > 1 ADMM_ERR_UNSUPPORTED while any share is above 0 (admm_hip_finalize checks
 *                                        the same once more; no sequence of calls reaches that check today).
 *   admm_hip_set_surface_reaction_depth  depth_min >= 0 (ADMM_ERR_ARG otherwise, NaN included).
 *   admm_hip_get_surface_reaction        the last frame's: dv [n_nodes][3] in the caller's node order, exactly 0.0 where nothing landed;
 *                                        one 64-byte record per contact in admm_hip_get_contacts' order {node, mesh (-1: the entry names
 *                                        none), tri (original index), corner[3] (caller's node ids), status, weight[3], share}, -1 and 0.0
 *                                        where the contact does not react; *count = K, records [capacity] receives the first
 *                                        min(K, capacity); info over all K.  Checks and behaves like the reaction reports: its own
 *                                        arguments, a host-only context, ADMM_ERR_STATE before the first step.  The counts are summed
 *                                        on the device (one one-wave launch); dv, K and the counts arrive behind one wait, the
 *                                        min(K, capacity) records behind a second: nothing beyond them is copied.  After
 *                                        a frame that ran with all shares zero: dv 0, no records.  Any output may be NULL.
 *   admm_hip_surface_reaction_query      context-free host evaluation of the shares and the ordered sums, the device's bits; needs no GPU:
 *                                        m3 [n_nodes][3] (a node's mass per component), f [K][3], corner [K][3], weight [K][3], share [K]
 *                                        -> dv [n_nodes][3].  A row with share 0 adds nothing (its corners are not read).  ADMM_ERR_ARG:
 *                                        n_nodes < 1, K < 0, a NULL pointer, dt not > 0, a share outside [0, 1], a corner of a row with
 *                                        share > 0 outside the nodes.
 *   admm_hip_debug_stable_sort           the feature's sort kernels alone: perm [n] = the stable ascending order of keys [n], every key in
 *                                        [0, key_bound), key_bound <= 2^31 - 1; one pass per 8 bits of key_bound - 1.  For tests.
 * Not covered: reactions of self-contacts, edge-edge contact, continuous detection, sharded contexts.                                      */
enum { ADMM_SURFACE_REACTING = 0, ADMM_SURFACE_UNOWNED = 1, ADMM_SURFACE_OTHER = 2, ADMM_SURFACE_SELF = 3 };
typedef struct admm_hip_surface_contact {
    int32_t node, mesh, tri, corner[3], status, pad_;
    double weight[3], share;
} admm_hip_surface_contact;
typedef struct admm_hip_surface_reaction_info {
    int64_t n_contacts, n_reacting, n_unowned, n_other, n_self;
} admm_hip_surface_reaction_info;
int admm_hip_set_surface_reaction(admm_hip_ctx *ctx, int mesh_id, double share);
int admm_hip_set_surface_reaction_depth(admm_hip_ctx *ctx, double depth_min);
int admm_hip_get_surface_reaction(admm_hip_ctx *ctx, double *dv, admm_hip_surface_contact *records, int64_t capacity, int64_t *count, admm_hip_surface_reaction_info *info);
int admm_hip_surface_reaction_query(int64_t n_nodes, const double *m3, int64_t K, const double *f, const int32_t *corner, const double *weight, const double *share,
                                    double dt, double *dv);
int admm_hip_debug_stable_sort(admm_hip_ctx *ctx, int64_t n, const int32_t *keys, int64_t key_bound, int32_t *perm);

/* ---- rigid bodies in the collision list, moved by their contacts ---------------------------------------------------------------------------
 * Extension, no reference counterpart; off unless asked for.  An entry of the collision list (a sphere, a box or a closed obstacle mesh)
 * becomes a rigid body with a mass and an inertia tensor.  Once per frame, after admm_hip_step's epilogue and the two-way contact and
 * before the velocity damping, the device takes the body's row {sum f, sum (point - c) x f} of admm_hip_entry_resultants(depth_min,
 * pivot = the body's own centre c) -- what its contacts exerted on the nodes -- applies the opposite to the body, integrates it and
 * keeps the new state; at the very start of the next admm_hip_step, before the body surfaces and the side latch, it writes the pose
 * into the entry's rows of the shape table (par, frame, framed, motion).  No host synchronisation, no atomics, fixed orders: two runs
 * give the same bits.  One definition, csrc/rigid.hpp, compiled without fused multiply-adds for the host and the device:
 *   state      c[3] centre of mass, q[4] = (w, x, y, z) unit quaternion, v[3], L[3] angular momentum about c in world axes
 *   one frame  F = -Fe, tau = -Te;  v' = v + dt (F / m + accel);  L' = L + dt tau;  R = R(q);  omega' = R (Jinv (R^T L'));
 *              c' = c + dt v';  h = (dt / 2) omega';  q' = normalise((1, h) / sqrt(1 + |h|^2) (x) q)  -- the Cayley transform, an exact
 *              rotation by 2 atan|h|, within (dt |omega|)^3 / 12 of dt |omega| per frame
 *   pose       frame = {R(q'), c'}, framed = R(q') is not exactly I, motion = {v', omega', c'}; a sphere's or a mesh's par[0..2] =
 *              par0 + (c' - c0), a box's par unchanged (its centre is the frame's pivot)
 * Launches per frame (csrc/kernels_rigid.hpp): rigid_pose_kernel at the start; behind the epilogue the reaction and attribution reports'
 * kernels, entry_count / scan / place, rigid_partial_kernel, rigid_reduce_kernel, rigid_integrate_kernel -- eager on the context's stream,
 * outside the captured graphs.  Every buffer is allocated by finalize or by the first admm_hip_add_rigid_body of a finalized context,
 * never by admm_hip_step.  A context without a body launches and uploads exactly what it did.  Because the pose is rewritten at every
 * step, a setter that uploads the host's (older) shape table between frames does not undo a body's motion.
 *   admm_hip_add_rigid_body   entry of the current list; inertia[6] = (xx, xy, xz, yy, yz, zz) about com in the entry's own unrotated
 *                             coordinates; com[3] in world coordinates; accel[3] a constant acceleration (gravity).  Before or after
 *                             finalize.  Order of the checks: ADMM_ERR_ARG the entry is out of range or a body already; its type is
 *                             FLOOR or CYLINDER (infinite shapes); it is a mesh that is a body or sheet surface; mass, inertia, com or
 *                             accel not finite, mass not > 0, inertia not positive definite; then ADMM_ERR_STATE contact attribution is
 *                             off; then ADMM_ERR_UNSUPPORTED world > 1 (a rank sees its share of the contacts only); then ADMM_ERR_ARG
 *                             the entry's frame is neither the identity (its pivot then becomes com) nor pivoted at com (a box: com
 *                             must be its pivot, the box's centre).  The orientation starts from the entry's R.  While a body exists,
 *                             admm_hip_enable_contact_attribution(ctx, 0) returns ADMM_ERR_STATE, admm_hip_set_shard with world > 1
 *                             ADMM_ERR_UNSUPPORTED, admm_hip_set_collision_shapes with a list of another length ADMM_ERR_STATE; with
 *                             the same length a body entry keeps its type (ADMM_ERR_ARG otherwise) and its params are ignored.
 *   admm_hip_set_rigid_depth  depth_min >= 0 of the contacts that load the bodies (default 0).
 *   admm_hip_get_rigid_state  one record per body, in the order they were added: the state, the derived omega, R (row-major) and the
 *                             entry's par, the last frame's applied F, tau and number of contacts.  One synchronisation; it also brings
 *                             the host's shape table up to date for the bodies' entries.  n_bodies must be the number of bodies.
 *   admm_hip_set_rigid_state  c, q, v, L of one body (a checkpoint, or a kick between frames); q is normalised unless |q|^2 is within
 *                             8 ulp of 1 (a q read back keeps its bits); omega is derived from the q given, which may differ in the
 *                             last bits from what the frame before left; F, tau and the count return to 0.  ADMM_ERR_ARG: not finite.
 *   admm_hip_set_rigid_accel  between any two frames; travels as a kernel argument with the next step.
 *   admm_hip_rigid_query      context-free host evaluation of one frame for one body, the device's bits; needs no GPU.
 * Not covered: bodies do not collide with each other or with static entries; no compound bodies of several entries; a node's whole
 * f_contact goes to the owner of its winning element (the last mover); the load is explicit and one frame behind -- the staggered
 * coupling is stable only while the body's mass is well above that of the nodes it touches; where it breaks is not measured.          */
typedef struct admm_hip_rigid_state {
    double c[3], q[4], v[3], L[3], omega[3], R[9], par[4], F[3], tau[3];
    int64_t count;
    int32_t entry, pad_;
} admm_hip_rigid_state;
int admm_hip_add_rigid_body(admm_hip_ctx *ctx, int entry, double mass, const double inertia[6], const double com[3], const double accel[3], int *body_id);
int admm_hip_set_rigid_depth(admm_hip_ctx *ctx, double depth_min);
int admm_hip_get_rigid_state(admm_hip_ctx *ctx, int n_bodies, admm_hip_rigid_state *out);
int admm_hip_set_rigid_state(admm_hip_ctx *ctx, int body, const double c[3], const double q[4], const double v[3], const double L[3]);
int admm_hip_set_rigid_accel(admm_hip_ctx *ctx, int body, const double accel[3]);
/* a body's constants as registered (accel: as last set), what admm_hip_rigid_query takes; any output may be NULL */
int admm_hip_get_rigid_body(admm_hip_ctx *ctx, int body, int *entry, int *type, double *mass, double inertia[6], double accel[3], double c0[3], double par0[4]);
int admm_hip_rigid_query(int type, double mass, const double inertia[6], const double accel[3], const double c0[3], const double par0[4],
                         const admm_hip_rigid_state *in, const double Fe[3], const double Te[3], int64_t count, double dt, admm_hip_rigid_state *out);

/* ---- rigid attachments: anchor batches fastened to rigid bodies -----------------------------------------------------------------------------
 * Extension, no reference counterpart; off unless asked for.  A whole ANCHOR batch is attached to one rigid body of the section above.
 * At the very start of every admm_hip_step, behind the bodies' pose and before anything reads a target, the device rewrites the batch's
 * targets from the body's record as the frame before left it; behind the epilogue, before the bodies are integrated, it adds the
 * reaction of the batch's active elements to the body's row, so a body is moved by what it carries as well as by what it touches.  No
 * host synchronisation, no atomics, fixed orders: two runs give the same bits.  One definition, csrc/attach.hpp, compiled without
 * fused multiply-adds for the host and the device:
 *   offset     r = R^T (t - c), on the host at attachment, from an element's target t and the body's c, R of that moment
 *   target     t = c + R r; recomputed from a derived offset it may differ from the target the offset came from in the last bits
 *   load       an element with active != 0: f = w^2 ((z - u) - x) (csrc/reaction.hpp) applied at z, its torque about the body's centre
 *              before this frame's integration; a released element (active == 0): six +0.0
 *   sum        per body over its attached elements in ascending (batch index, element in admm_hip_read_local's order), in reaction.hpp's
 *              two-stage order (64-element blocks, then 256 lanes)
 *   combined   only a body that carries a batch: Fe = Fc + Fa, Te = Tc + Ta, one rounded add each, then the rule of the section above
 *              unchanged; a body without a batch keeps the bits it had.  admm_hip_rigid_state.count stays the number of contacts, F and
 *              tau are the total applied.
 * Launches per frame (csrc/kernels_attach.hpp): attach_targets_kernel behind rigid_pose_kernel; attach_partial_kernel and
 * attach_reduce_kernel before rigid_integrate_kernel -- eager on the context's stream, outside the captured graphs, which keep working
 * because a batch's targets keep their address.  Every buffer is allocated by finalize or by the attaching call on a finalized context,
 * never by admm_hip_step.  A context without an attached batch launches and uploads exactly what it did.
 *   admm_hip_attach_anchors      before or after finalize.  local [n_total][3]: the elements' offsets in the body's own coordinates, in
 *                                the order the batch was added; NULL: derived from the batch's current targets (a batch added without
 *                                targets: its nodes' positions) and the body's current pose (one synchronisation after finalize).
 *                                Order of the checks: ADMM_ERR_ARG the batch is not an anchor batch; the body is not a rigid body; the
 *                                batch is attached already; an offset is not finite; then ADMM_ERR_UNSUPPORTED world > 1 (which
 *                                admm_hip_add_rigid_body refuses too; the message names the batch).  A body that carries a batch still
 *                                needs what admm_hip_add_rigid_body needs: contact attribution on and world == 1.  A context with a body,
 *                                attachments and no collision batch at all steps: the body is then loaded by its attachments alone.
 *   admm_hip_detach_anchors      the targets stay where the last frame put them; the batch is a plain moving-anchor batch again.
 *                                ADMM_ERR_ARG: not an anchor batch, or not attached.
 *   admm_hip_get_attachment      body (-1: not attached), local [n_total][3] (zeros when not attached), targets [n_total][3] as the
 *                                device holds them now (one synchronisation); any output may be NULL.  A released element's target is
 *                                its node's position, which the anchor kernel stores there in every local step.
 *   admm_hip_get_attachment_load the last frame's attachment row per body, Fa [n][3] and Ta [n][3] about the centre before that frame's
 *                                integration, and the number of active attached elements; as the nodes felt it, the body received the
 *                                opposite.  n_bodies must be the number of bodies.  Zeros before the first frame and for a body without
 *                                a batch.
 *   admm_hip_attachment_query    context-free host evaluation, the device's bits; needs no GPU.  Target half (targets != NULL):
 *                                targets [n][3] from c[3], R[9] (row-major) and local [n][3].  Sum half (row6 or n_active != NULL): the
 *                                six sums {sum f, sum (point - pivot) x f} over the n elements in the device's order, from f [n][3] and
 *                                point [n][3] -- what admm_hip_batch_reaction and admm_hip_read_local's z return -- active [n] (NULL: all
 *                                active; a released element adds six +0.0) and pivot[3] (NULL: the origin).
 * While a batch is attached, admm_hip_update_anchors with targets != NULL returns ADMM_ERR_STATE (the next step would overwrite them);
 * the flags alone stay allowed and take effect as before.  admm_hip_set_rigid_state simply moves the attached targets at the next step.
 * Limits: whole batches only; one body per batch; no joints between bodies; not available under sharding.  The coupling is explicit and
 * staggered like the contact load -- the body feels this frame's reaction in the next -- and is stable only while the body is well
 * heavier than the nodes fastened to it; where it breaks is not measured.  Linear momentum balances up to the solve's residual; angular
 * momentum is not exact, because the reaction is applied at the target z, not at the node.                                              */
int admm_hip_attach_anchors(admm_hip_ctx *ctx, int batch, int body, const double *local);
int admm_hip_detach_anchors(admm_hip_ctx *ctx, int batch);
int admm_hip_get_attachment(admm_hip_ctx *ctx, int batch, int *body, double *local, double *targets);
int admm_hip_get_attachment_load(admm_hip_ctx *ctx, int n_bodies, double *Fa, double *Ta, int64_t *n_active);
int admm_hip_attachment_query(int64_t n, const double c[3], const double R[9], const double *local, double *targets, const double *f, const double *point,
                              const int32_t *active, const double pivot[3], double *row6, int64_t *n_active);

#ifdef __cplusplus
}
#endif
#endif
