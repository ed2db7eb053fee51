// Force.hpp -- host-side mirror of the reference's force classes
// (deps/admm-elastic-sca/src/system/Force.hpp, TetForce.hpp, TriangleForce.hpp,
// BendForce.hpp, AnchorForce.hpp, CollisionForce.hpp, ExplicitForce.hpp and
// src/collision/*.hpp): same class names, constructor signatures, virtuals and
// public data members, so scene code that builds forces and pushes them into
// System::forces compiles unchanged.  The reference's per-class headers
// (TetForce.hpp, AnchorForce.hpp ...) exist next to this file and forward here.
//
// The plugin surface is the reference's (Force.hpp:37-57):
//     subclass admm::Force, implement get_selector() + project(), push it into system->forces.
// Built-in classes are *descriptions* (kind, node ids, parameters): their
// initialize / get_selector / project run inside libadmm_hip.so, one HIP kernel
// per kind.  A user-written subclass is host code by nature: System collects its
// selector rows once, the device evaluates D_i x for them every ADMM iteration,
// project() runs on the host, and z - u goes back into the device-side
// right-hand side (admm_hip_add_generic_batch).  Same for a user-written
// CollisionShape (its CollisionForce then projects on the host) and a
// user-written ExplicitForce (applied on the host before the frame is uploaded).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>

#include "Vec.hpp"
#include "admm_hip.h"
#include "admm_kinds.h"

namespace admm {

class Force {
public:
    int global_idx;  // position of this force's first row in u / z (built-ins: compact rows, filled by System::initialize;
                     // user forces: the weights.size() they saw in get_selector, i.e. their offset among the user rows)
    double weight;   // computed by the force from its stiffness (built-ins: filled by System::initialize)
    Force() : global_idx(0), weight(0.f) {}
    virtual ~Force() {}
    // Force.hpp:46-55
    virtual void initialize(const Eigen::VectorXd & /*x*/, const Eigen::VectorXd & /*v*/, const Eigen::VectorXd & /*masses*/, const double /*timestep*/) {}
    virtual void get_selector(const Eigen::VectorXd &x, std::vector<Eigen::Triplet<double> > &triplets, std::vector<double> &weights) = 0;
    virtual void project(double dt, const Eigen::VectorXd &Dx, Eigen::VectorXd &u, Eigen::VectorXd &z) const = 0;
    virtual void set_eps(double) {}
    // ---- mirror only ----
    // >= 0: a built-in kind with a HIP kernel; -1: user code, projected on the host
    virtual int kind() const { return -1; }
    // node ids, ADMM_KIND_PARAMS[kind] parameters (admm_kinds.h)
    virtual void describe(int *, double *) const {}
    // the class whose kernel kind() names; a subclass of a built-in that does not say so is refused by System::initialize
    virtual const std::type_info &device_type() const { return typeid(void); }
};

// A force whose Force::initialize / get_selector / project run inside libadmm_hip.so (no host arithmetic exists for it).
class DeviceForce : public Force {
public:
    void get_selector(const Eigen::VectorXd &, std::vector<Eigen::Triplet<double> > &, std::vector<double> &) { host_call("get_selector"); }
    void project(double, const Eigen::VectorXd &, Eigen::VectorXd &, Eigen::VectorXd &) const { host_call("project"); }
private:
    static void host_call(const char *what) {
        std::fprintf(stderr, "\n**Solver Error: %s() of a built-in force was called on the host; built-in forces run on the GPU inside System::initialize()/step()\n", what);
        std::abort();
    }
};
#define ADMM_DEVICE_FORCE(Class, Kind) int kind() const { return Kind; } const std::type_info &device_type() const { return typeid(Class); }

class Spring : public DeviceForce {
public:
    Spring(int idx0_, int idx1_, double stiffness_) : idx0(idx0_), idx1(idx1_), stiffness(stiffness_), rest_length(0) {}
    ADMM_DEVICE_FORCE(Spring, ADMM_KIND_SPRING)
    void describe(int *idx, double *p) const { idx[0] = idx0; idx[1] = idx1; p[0] = stiffness; }
    int idx0, idx1;
    double stiffness, rest_length;
};

class LinearTetStrain : public DeviceForce {
public:
    LinearTetStrain(int i0, int i1, int i2, int i3, double stiffness_, double weight_scale_ = 1.f)
        : stiffness(stiffness_), volume(0.0), weight_scale(weight_scale_) { idx[0] = i0; idx[1] = i1; idx[2] = i2; idx[3] = i3; }
    ADMM_DEVICE_FORCE(LinearTetStrain, ADMM_KIND_TET_LINEAR)
    void describe(int *id, double *p) const { for (int i = 0; i < 4; ++i) id[i] = idx[i]; p[0] = stiffness; }
    int idx[4];
    double stiffness, volume, weight_scale;
};

class TetVolume : public DeviceForce {
public:
    TetVolume(int i0, int i1, int i2, int i3, double stiffness_, double limit_min_, double limit_max_)
        : stiffness(stiffness_), rest_volume(0.0), limit_min(limit_min_), limit_max(limit_max_) { idx[0] = i0; idx[1] = i1; idx[2] = i2; idx[3] = i3; }
    ADMM_DEVICE_FORCE(TetVolume, ADMM_KIND_TET_VOLUME)
    void describe(int *id, double *p) const { for (int i = 0; i < 4; ++i) id[i] = idx[i]; p[0] = stiffness; p[1] = limit_min; p[2] = limit_max; }
    int idx[4];
    double stiffness, rest_volume, limit_min, limit_max;
};

// type "nh"/"0" -> Neo-Hookean, "stvk"/"1" -> St. Venant-Kirchhoff (TetForce.hpp:118-121)
class HyperElasticTet : public DeviceForce {
public:
    HyperElasticTet(int i0, int i1, int i2, int i3, double mu_, double lambda_, int max_iterations_, std::string type_)
        : mu(mu_), lambda(lambda_), volume(0.0), max_iterations(max_iterations_) {
        idx[0] = i0; idx[1] = i1; idx[2] = i2; idx[3] = i3;
        type = 0; if (type_ == "stvk" || type_ == "1") type = 1;
    }
    int kind() const { return type == 1 ? ADMM_KIND_TET_STVK : ADMM_KIND_TET_NH; }
    const std::type_info &device_type() const { return typeid(HyperElasticTet); }
    void describe(int *id, double *p) const { for (int i = 0; i < 4; ++i) id[i] = idx[i]; p[0] = mu; p[1] = lambda; p[2] = max_iterations; }
    int idx[4];
    int type;
    double mu, lambda, volume;
    int max_iterations;
};

class LimitedTriangleStrain : public DeviceForce {
public:
    LimitedTriangleStrain(int id0_, int id1_, int id2_, double stiffness_, double limit_min_, double limit_max_, bool strain_limiting_ = true)
        : id0(id0_), id1(id1_), id2(id2_), stiffness(stiffness_), limit_min(limit_min_), limit_max(limit_max_), area(0), strain_limiting(strain_limiting_) {}
    ADMM_DEVICE_FORCE(LimitedTriangleStrain, ADMM_KIND_TRI_STRAIN)
    void describe(int *id, double *p) const { id[0] = id0; id[1] = id1; id[2] = id2; p[0] = stiffness; p[1] = limit_min; p[2] = limit_max; p[3] = strain_limiting ? 1.0 : 0.0; }
    int id0, id1, id2;
    double stiffness, limit_min, limit_max, area;
    bool strain_limiting;
};

// TriangleForce.hpp:126-133: area-preserving triangle; inherits the strain triangle's rest data and weight
class TriArea : public LimitedTriangleStrain {
public:
    TriArea(int id0_, int id1_, int id2_, double stiffness_, int iters_, double limit_min_, double limit_max_)
        : LimitedTriangleStrain(id0_, id1_, id2_, stiffness_, limit_min_, limit_max_), iters(iters_) {}
    ADMM_DEVICE_FORCE(TriArea, ADMM_KIND_TRI_AREA)
    void describe(int *id, double *p) const { id[0] = id0; id[1] = id1; id[2] = id2; p[0] = stiffness; p[1] = iters; p[2] = limit_min; p[3] = limit_max; }
    int iters;
};

// TriangleForce.hpp:106-124: Fung skin membrane, prox by L-BFGS (2 variables, maxIter 10, gradTol 1e-6)
class FungTriangle : public DeviceForce {
public:
    FungTriangle(int id0_, int id1_, int id2_, double mu_, double limit_min_, double limit_max_)
        : id0(id0_), id1(id1_), id2(id2_), mu(mu_), limit_min(limit_min_), limit_max(limit_max_), area(0) {}
    ADMM_DEVICE_FORCE(FungTriangle, ADMM_KIND_TRI_FUNG)
    void describe(int *id, double *p) const { id[0] = id0; id[1] = id1; id[2] = id2; p[0] = mu; p[1] = limit_min; p[2] = limit_max; }
    int id0, id1, id2;
    double mu, limit_min, limit_max, area;
};

class BendForce : public DeviceForce {
public:
    BendForce(int i0, int i1, int i2, int i3, double stiffness_) : stiffness(stiffness_) { idx[0] = i0; idx[1] = i1; idx[2] = i2; idx[3] = i3; weight = std::sqrt(stiffness); }
    ADMM_DEVICE_FORCE(BendForce, ADMM_KIND_BEND)
    void describe(int *id, double *p) const { for (int i = 0; i < 4; ++i) id[i] = idx[i]; p[0] = stiffness; }
    int idx[4];
    double stiffness;
};

class StaticAnchor : public DeviceForce {
public:
    StaticAnchor(int idx_, double use_weight_ = -1.0) : idx(idx_), use_weight(use_weight_) {
        if (use_weight_ > 0.0) weight = use_weight_; else weight = 1000.f;
    }
    ADMM_DEVICE_FORCE(StaticAnchor, ADMM_KIND_ANCHOR)
    void describe(int *id, double *p) const { id[0] = idx; p[0] = weight; p[1] = 1.0; }
    int idx;
    double use_weight;
    Vector3d pos;
};

class MovingAnchor;
class CollisionShape;
class ControlPoint {
public:
    ControlPoint() : active(true), anchorForce(0) { pos.setZero(); }
    ControlPoint(Vector3d pos_) : pos(pos_), active(true), anchorForce(0) {}
    Vector3d pos;
    bool active;
    MovingAnchor *anchorForce;
};

class MovingAnchor : public DeviceForce {
public:
    MovingAnchor(int idx_, std::shared_ptr<ControlPoint> p_, double use_weight_ = -1.0) : idx(idx_), point(p_) {
        point->anchorForce = this;
        if (use_weight_ > 0.0) weight = use_weight_; else weight = 1000.f;
    }
    ADMM_DEVICE_FORCE(MovingAnchor, ADMM_KIND_ANCHOR)
    void describe(int *id, double *p) const { id[0] = idx; p[0] = weight; p[1] = point->active ? 1.0 : 0.0; }
    int idx;
    std::shared_ptr<ControlPoint> point;
    // Extension, no reference counterpart (admm_hip_attach_anchors): a CollisionShape that is a rigid body (rigid_mass > 0) -- the anchor
    // is fastened to it.  The device then moves the control point with the body's pose at the start of every step and loads the body
    // with the anchor's reaction; point->pos gives the offset once, at System::initialize, is not uploaded while attached and is
    // refreshed from the device only by System::attachment_targets().  point->active still releases the anchor.  Null (default): a
    // plain moving anchor.  Consecutive moving anchors with the same body form one device batch.
    std::shared_ptr<CollisionShape> body;
};

namespace helper {
// AnchorForce.hpp:31-48
static inline Vector3d smooth_move(double total_elapsed_dt, double start_dt, double end_dt, Vector3d start, Vector3d end) {
    if (total_elapsed_dt < start_dt) return start;
    double tRatio = (total_elapsed_dt - start_dt) / (end_dt - start_dt);
    if (tRatio > 1.0) return end;
    Vector3d displacement = end - start;
    return (start + (3.0 * tRatio * tRatio - 2.0 * tRatio * tRatio * tRatio) * displacement);
}
static inline Vector3d linear_move(double total_elapsed_dt, double start_dt, double end_dt, Vector3d start, Vector3d end) {
    if (total_elapsed_dt < start_dt) return start;
    double tRatio = (total_elapsed_dt - start_dt) / (end_dt - start_dt);
    if (tRatio > 1.0) return end;
    Vector3d displacement = end - start;
    return (start + displacement);
}
} // namespace helper

// deps/admm-elastic-sca/src/collision/: shapes tested in list order by CollisionForce.  The three analytic shapes have a
// device form (shape_type() >= 0); a user-written shape implements isColliding / projectOut like in the reference
// (CollisionShape.hpp:34-38) and makes its CollisionForce a host-projected force.
class CollisionShape {
public:
    CollisionShape(Vector3d shapeCenter) { center = shapeCenter; }
    virtual ~CollisionShape() {}
    virtual double isColliding(Vector3d pos) const = 0;            // > 0 inside
    virtual Vector3d projectOut(const Vector3d currPos) const = 0;
    virtual int shape_type() const { return -1; }                  // ADMM_SHAPE_*, -1 = user code
    virtual double shape_radius() const { return 0.0; }
    Vector3d center;
    // Extension, no reference counterpart: the Coulomb coefficient of contacts with this shape (admm_hip_set_collision_friction), for
    // shapes with a device form; may change between frames.  System::initialize refuses it on a user-written (host-projected) shape
    // and on a CollisionBody (a moving simulated surface: its velocity would be needed).
    double friction = 0.0;
    // ... and the shape's rigid motion as the friction rule sees it (admm_hip_set_collision_motion): linear and angular velocity and the
    // pivot, world coordinates, default zero; a contact with friction > 0 then sticks to the moving surface.  Moving `center` between
    // frames does not set it.  Must stay zero on a CollisionBody (the library refuses it there).
    Vector3d lin_velocity = Vector3d(0, 0, 0), ang_velocity = Vector3d(0, 0, 0), pivot = Vector3d(0, 0, 0);
    // ... and the shape's rigid frame (admm_hip_set_collision_frames): the shape, as its other members describe it, rotated by
    // `orientation` (3x3, row-major, a rotation; default the identity) about `orientation_pivot`, world coordinates.  May change between
    // frames; turning it does not set ang_velocity.  The device applies it; the built-in shapes' host isColliding / projectOut do not,
    // except CollisionBox's.  Must stay the identity on a CollisionBody (the library refuses it there).
    double orientation[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    Vector3d orientation_pivot = Vector3d(0, 0, 0);
    // the twelve doubles of the ABI, about `about`
    void frame(const Vector3d &about, double *f) const {
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) f[3 * i + j] = orientation[i][j];
        for (int j = 0; j < 3; ++j) f[9 + j] = about[j];
    }
    virtual Vector3d frame_pivot() const { return orientation_pivot; }
    // ... and a rigid body (admm_hip_add_rigid_body; a sphere, a box or a closed obstacle mesh): rigid_mass > 0 makes the shape one, moved
    // on the device by the reaction of its contacts.  rigid_inertia = (xx, xy, xz, yy, yz, zz) about the centre of mass in the shape's own
    // unrotated coordinates, rigid_accel a constant acceleration (gravity).  The centre of mass is `center` for a sphere and the frame's
    // pivot otherwise, unless rigid_com_set names rigid_com.  Read once, by System::initialize, behind the frames; needs
    // System::settings.contact_attribution.  From then on the device owns the shape's pose: System::rigid_state() reports it, and
    // `center`, `orientation` and the motion members are no longer read for it.
    double rigid_mass = 0.0, rigid_inertia[6] = {0, 0, 0, 0, 0, 0};
    Vector3d rigid_accel = Vector3d(0, 0, 0), rigid_com = Vector3d(0, 0, 0);
    bool rigid_com_set = false;
};
class CollisionFloor : public CollisionShape {
public:
    CollisionFloor(Vector3d shapeCenter) : CollisionShape(shapeCenter), radius(0) {}
    double isColliding(Vector3d pos) const { return center[1] - pos[1]; }
    Vector3d projectOut(const Vector3d currPos) const { return Vector3d(currPos[0], center[1], currPos[2]); }
    int shape_type() const { return typeid(*this) == typeid(CollisionFloor) ? ADMM_SHAPE_FLOOR : -1; }
    double radius;
};
class CollisionSphere : public CollisionShape {
public:
    CollisionSphere(Vector3d shapeCenter, double sphRadius) : CollisionShape(shapeCenter), radius(sphRadius) {}
    double isColliding(Vector3d pos) const { return radius - (pos - center).norm(); }
    Vector3d projectOut(const Vector3d currPos) const { Vector3d d = currPos - center; return center + radius * (d / d.norm()); }
    int shape_type() const { return typeid(*this) == typeid(CollisionSphere) ? ADMM_SHAPE_SPHERE : -1; }
    double shape_radius() const { return radius; }
    double radius;
};
// axis parallel to z through (center.x, center.y); CollisionCylinder.hpp:48-50 drops center.z
class CollisionCylinder : public CollisionShape {
public:
    CollisionCylinder(Vector3d shapeCenter, Vector3d /*cylScale*/, double cylRadius) : CollisionShape(Vector3d(shapeCenter[0], shapeCenter[1], 0)), radius(cylRadius), length(0) {}
    double isColliding(Vector3d pos) const { return radius - (Vector3d(pos[0], pos[1], 0) - center).norm(); }
    Vector3d projectOut(const Vector3d currPos) const {
        Vector3d flat(currPos[0], currPos[1], 0);
        Vector3d d = flat - center;
        return (center + radius * (d / d.norm())) + Vector3d(0, 0, currPos[2]);
    }
    int shape_type() const { return typeid(*this) == typeid(CollisionCylinder) ? ADMM_SHAPE_CYLINDER : -1; }
    double shape_radius() const { return radius; }
    double radius, length;
};

// Extension, no reference counterpart: a box of half extents `half` centred at `center`, turned by `orientation` about its centre
// (ADMM_SHAPE_BOX; orientation_pivot is not used: the centre is the pivot).  isColliding / projectOut evaluate the library's rule on
// the host (admm_hip_shape_query: the code the device runs): isColliding is +1 where the box would move the point and -1 elsewhere.
class CollisionBox : public CollisionShape {
public:
    CollisionBox(Vector3d shapeCenter, Vector3d halfExtents) : CollisionShape(shapeCenter), half(halfExtents) {}
    double isColliding(Vector3d pos) const { double o[3]; return query(pos, o) ? 1.0 : -1.0; }
    Vector3d projectOut(const Vector3d currPos) const { double o[3]; query(currPos, o); return Vector3d(o[0], o[1], o[2]); }
    int shape_type() const { return typeid(*this) == typeid(CollisionBox) ? ADMM_SHAPE_BOX : -1; }
    Vector3d frame_pivot() const { return center; }
    Vector3d half;
private:
    bool query(const Vector3d &p, double *o) const {
        const double par[4] = {half[0], half[1], half[2], 0.0}, q[3] = {p[0], p[1], p[2]};
        double f[12];
        frame(center, f);
        int32_t moved = 0;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        admm_hip_shape_query(ADMM_SHAPE_BOX, par, f, 1, q, o, &moved);
        return moved != 0;
    }
};

// Extension, no reference counterpart: a closed triangle mesh (verts [nv][3], tris [nt][3], counter-clockwise seen from outside)
// translated by `center`.  isColliding / projectOut evaluate the library's query on the host (admm_hip_mesh_query: +distance
// inside, -distance outside; the closest point); as the list's ADMM_SHAPE_MESH entry the device runs the same code.  The mesh is
// validated and its BVH built once here; System registers it with its context before initialize (once per distinct mesh).
// Invalid meshes throw std::runtime_error with the library's message.  set_vertices deforms it (the same topology, new positions:
// admm_hip_mesh_set_vertices) and bumps `version`; System's step() hands a changed mesh to its context (admm_hip_update_collision_mesh).
// With a half thickness > 0 (the second constructor) the surface may be open -- a sheet, a terrain patch, a half pipe -- and collides as a
// thick shell (admm_hip_mesh_create_open): isColliding then returns r - distance (-inf beyond r) and projectOut the point after the shell
// rule.  `half_thickness` may be changed between frames; System's step() hands a change to its context.
class CollisionMesh : public CollisionShape {
public:
    CollisionMesh(Vector3d shapeCenter, const std::vector<double> &verts, const std::vector<int> &tris, double half_thickness_) : CollisionShape(shapeCenter), vertices(verts), version(0), half_thickness(half_thickness_) {
        std::vector<int32_t> t(tris.begin(), tris.end());
        char err[512] = {0};
        admm_hip_mesh *m = nullptr;
        if (admm_hip_mesh_create_open(&m, (int)(verts.size() / 3), verts.data(), (int)(t.size() / 3), t.data(), half_thickness_, err, (int)sizeof err) != ADMM_OK)
            throw std::runtime_error(std::string("CollisionMesh: ") + err);
        mesh = std::shared_ptr<admm_hip_mesh>(m, admm_hip_mesh_destroy);
    }
    CollisionMesh(Vector3d shapeCenter, const std::vector<double> &verts, const std::vector<int> &tris) : CollisionShape(shapeCenter), vertices(verts), version(0) {
        std::vector<int32_t> t(tris.begin(), tris.end());
        char err[512] = {0};
        admm_hip_mesh *m = nullptr;
        if (admm_hip_mesh_create(&m, (int)(verts.size() / 3), verts.data(), (int)(t.size() / 3), t.data(), err, (int)sizeof err) != ADMM_OK)
            throw std::runtime_error(std::string("CollisionMesh: ") + err);
        mesh = std::shared_ptr<admm_hip_mesh>(m, admm_hip_mesh_destroy);
    }
    // new positions [nv][3] for the same triangles; a refused update throws std::runtime_error and leaves the mesh as it was
    void set_vertices(const std::vector<double> &verts) {
        char err[512] = {0};
        if (admm_hip_mesh_set_vertices(mesh.get(), (int)(verts.size() / 3), verts.data(), err, (int)sizeof err) != ADMM_OK)
            throw std::runtime_error(std::string("CollisionMesh::set_vertices: ") + err);
        vertices = verts;
        ++version;
    }
    // one velocity per vertex [nv][3] for the friction rule (admm_hip_set_collision_mesh_velocity), an empty vector: none again; System's
    // step() hands a change to its context.  Throws std::runtime_error for another count.
    void set_vertex_velocities(const std::vector<double> &vel) {
        if (!vel.empty() && vel.size() != vertices.size()) throw std::runtime_error("CollisionMesh::set_vertex_velocities: " + std::to_string(vel.size() / 3) + " velocities given, the mesh has " + std::to_string(vertices.size() / 3) + " vertices");
        velocities = vel;
        ++vel_version;
    }
    double isColliding(Vector3d pos) const { double pr[3], sd; query(pos, pr, sd); return sd; }
    Vector3d projectOut(const Vector3d currPos) const { double pr[3], sd; query(currPos, pr, sd); return Vector3d(pr[0], pr[1], pr[2]); }
    int shape_type() const { return typeid(*this) == typeid(CollisionMesh) ? ADMM_SHAPE_MESH : -1; }
    std::shared_ptr<admm_hip_mesh> mesh;
    std::vector<double> vertices;          // the current positions
    long version;                          // set_vertices calls so far
    std::vector<double> velocities;        // the vertices' velocities (empty: none)
    long vel_version = 0;                  // set_vertex_velocities calls so far
    double half_thickness = 0.0;           // 0: a closed mesh; > 0: an open surface, a shell of this half thickness (the host query uses the value at construction)
    // an open mesh only: > 0: side memory with this reach (admm_hip_set_collision_mesh_side_memory: every node remembers the side of the
    // surface it is on and is put back there when it crosses within a frame); read at System::initialize, where a force that projects on
    // the host refuses it (the sides live in the context)
    double side_reach = 0.0;
private:
    void query(const Vector3d &p, double *pr, double &sd) const {
        const double t[3] = {center[0], center[1], center[2]}, q[3] = {p[0], p[1], p[2]};
        admm_hip_mesh_query(mesh.get(), t, 1, q, pr, &sd);
    }
};

// Extension, no reference counterpart: the closed boundary surface of a simulated body, triangles tris [nt][3] of global node ids
// inside [node_first, node_first + node_count) (meshgen.tet_surface's output, for example), counter-clockwise seen from outside.
// System registers it with its context before initialize (admm_hip_add_body_surface); the device then rebuilds it from the nodes
// at the start of every step, and the body's own nodes ignore it.  It has no host evaluation (it needs the nodes' positions):
// a CollisionForce that projects on the host (a user-written shape in its list) refuses it at System::initialize.
class CollisionBody : public CollisionShape {
public:
    CollisionBody(int node_first_, int node_count_, const std::vector<int> &tris_) : CollisionShape(Vector3d(0, 0, 0)), node_first(node_first_), node_count(node_count_), tris(tris_) {}
    double isColliding(Vector3d) const { return -1.0; }
    Vector3d projectOut(const Vector3d currPos) const { return currPos; }
    int shape_type() const { return typeid(*this) == typeid(CollisionBody) ? ADMM_SHAPE_MESH : -1; }
    int node_first, node_count;
    std::vector<int> tris;
    // the Coulomb coefficient of contacts with this surface (admm_hip_set_body_surface_friction): a property of the body, whatever list
    // names it; the surface's velocity at a contact is its nodes'.  `friction` (the per-entry coefficient) stays refused on a CollisionBody.
    double surface_friction = 0.0;
    // {r, reach, rest_radius}, r > 0: the body's surface nodes meet this surface too, outside what is near them in the rest shape
    // (admm_hip_set_body_self_collision); read at System::initialize, where a force that projects on the host refuses it.  (A
    // CollisionSheet has a flag of the same name instead: admm_hip_set_sheet_self_collision.)
    double self_collision[3] = {0.0, 0.0, 0.0};
    // two-way contact (admm_hip_set_surface_reaction): the share in [0, 1] of a contact's reaction that the corners of the triangle it
    // landed on receive; 0: none.  Needs System::settings.contact_attribution; read at every step(), so it may change between frames.
    double reaction_share = 0.0;
};

// Extension, no reference counterpart: CollisionBody for an open surface of simulated nodes such as a cloth (admm_hip_add_sheet_surface):
// a thick shell of half thickness r that follows its nodes and is ignored by them -- or, with self_collision set before initialize, met by
// them outside their 1-ring (cloth self-collision); every rule and refusal of a CollisionBody holds.
class CollisionSheet : public CollisionBody {
public:
    CollisionSheet(int node_first_, int node_count_, const std::vector<int> &tris_, double half_thickness_) : CollisionBody(node_first_, node_count_, tris_), half_thickness(half_thickness_) {}
    int shape_type() const { return typeid(*this) == typeid(CollisionSheet) ? ADMM_SHAPE_MESH : -1; }
    double half_thickness;
    bool self_collision = false;      // the sheet's own nodes meet it outside their 1-ring (admm_hip_set_sheet_self_collision); read at System::initialize
    double side_reach = 0.0;          // > 0: side memory with this reach for the nodes that do not own the sheet (admm_hip_set_collision_mesh_side_memory); read at System::initialize
};

// One force over ALL nodes (CollisionForce.hpp:31-46).  With analytic shapes only: a device batch with one element per
// node.  With a user-written shape in the list the shapes' virtuals have to run on the host, so the force describes itself
// like any user force: identity rows (CollisionForce.cpp:29-36) and the projection loop of :38-70.
class CollisionForce : public Force {
public:
    CollisionForce(std::vector<std::shared_ptr<CollisionShape> > &collShapes, double use_weight = 32.0) : collisionShapes(collShapes), Di_rows(0), n_nodes(0) { weight = use_weight; }
    bool device_shapes() const { for (size_t j = 0; j < collisionShapes.size(); ++j) if (collisionShapes[j]->shape_type() < 0) return false; return true; }
    int kind() const { return (typeid(*this) == typeid(CollisionForce) && device_shapes()) ? ADMM_KIND_COLLISION : -1; }
    const std::type_info &device_type() const { return typeid(CollisionForce); }
    void initialize(const Eigen::VectorXd &x, const Eigen::VectorXd &, const Eigen::VectorXd &, const double) { n_nodes = (int)x.size() / 3; }
    void get_selector(const Eigen::VectorXd &x, std::vector<Eigen::Triplet<double> > &triplets, std::vector<double> &weights) {
        global_idx = (int)weights.size();
        Di_rows = (int)x.size();
        for (int i = 0; i < Di_rows; ++i) { triplets.push_back(Eigen::Triplet<double>(i + global_idx, i, 1.0)); weights.push_back(weight); }
    }
    void project(double, const Eigen::VectorXd &Dx, Eigen::VectorXd &u, Eigen::VectorXd &z) const {
        for (int i = 0; i < Di_rows; i += 3) {
            const int g = global_idx + i;
            Vector3d free_pos(Dx[g] + u[g], Dx[g + 1] + u[g + 1], Dx[g + 2] + u[g + 2]);
            Vector3d point = free_pos;
            for (size_t j = 0; j < collisionShapes.size(); ++j) if (collisionShapes[j]->isColliding(point) > 0) point = collisionShapes[j]->projectOut(point);
            for (int c = 0; c < 3; ++c) { u[g + c] += (Dx[g + c] - point[c]); z[g + c] = point[c]; }
        }
    }
    std::vector<std::shared_ptr<CollisionShape> > collisionShapes;
    int Di_rows, n_nodes;
};

// ExplicitForce.hpp:51-59: constant acceleration on all nodes or on an index subset.  ExplicitForce and WindForce themselves
// run on the device; a user-written subclass overrides project() and is applied on the host at the start of System::step().
class ExplicitForce {
public:
    ExplicitForce(std::vector<int> indices_ = std::vector<int>(0)) { indices = indices_; }
    ExplicitForce(Vector3d direction_, std::vector<int> indices_ = std::vector<int>(0)) { direction = direction_; indices = indices_; }
    virtual ~ExplicitForce() {}
    // ExplicitForce.cpp:29-39 (what a subclass inherits when it does not override)
    virtual void project(double dt, Eigen::VectorXd &x, Eigen::VectorXd &v, Eigen::VectorXd & /*m*/) const {
        if (indices.empty()) for (std::ptrdiff_t i = 0; i < (std::ptrdiff_t)x.size() / 3; ++i) { for (int c = 0; c < 3; ++c) v[3 * i + c] += dt * direction[c]; }
        else for (size_t q = 0; q < indices.size(); ++q) for (int c = 0; c < 3; ++c) v[3 * (std::ptrdiff_t)indices[q] + c] += dt * direction[c];
    }
    virtual int explicit_type() const { return ADMM_EXPLICIT_CONST; }
    virtual const std::vector<int> &index_list() const { return indices; }
    bool on_device() const { return typeid(*this) == device_class(); }
    virtual const std::type_info &device_class() const { return typeid(ExplicitForce); }
    Vector3d direction;
    std::vector<int> indices;
};

// ExplicitForce.hpp:62-71: aerodynamic drag on a list of triangles; direction is host-mutable
class WindForce : public ExplicitForce {
public:
    WindForce(std::vector<int> &tris_) : tris(tris_) { this->direction = Vector3d(0, 0, 0); }
    void project(double, Eigen::VectorXd &, Eigen::VectorXd &, Eigen::VectorXd &) const {
        std::fprintf(stderr, "\n**Solver Error: WindForce::project() runs on the GPU; a subclass must override project()\n");
        std::abort();
    }
    int explicit_type() const { return ADMM_EXPLICIT_WIND; }
    const std::vector<int> &index_list() const { return tris; }
    const std::type_info &device_class() const { return typeid(WindForce); }
    std::vector<int> tris;
};

} // namespace admm
