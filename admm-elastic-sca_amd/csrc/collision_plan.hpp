// collision_plan.hpp -- what the host decides about the collision meshes before anything is launched or uploaded, as pure functions on
// small arrays.  Free of HIP (tests/cpp/collision_plan.cpp includes this header alone):
//   collision_form_of   which kernels the collision batches launch for a shape list (launch.inc: collision_form), in one pass over it
//   plan_mesh_tables    the per-mesh and per-node tables that finalize uploads beside d_meshes (upload.inc: upload_all)
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "dev_types.hpp"

namespace admm_lib {

// ---- the form of a list -------------------------------------------------------------------------------------------------------------
// what the form depends on in a registered mesh (ctx.hpp CollisionMesh): is it a body surface, its half thickness (> 0: open), does the
// sheet collide with itself, the reach of its side memory (0: none), the half gap of a body's self-collision (body_self[0]; 0: off), a
// body surface's friction coefficient, and whether an obstacle has vertex velocities in effect
struct MeshFacts { bool body; double thickness; bool self_collision; double side_reach, body_self_r, body_mu; bool has_vel; };

// form: 0 the frictionless kernels, 1 the friction form, 2 its moving form, 3 the framed form, 4 the shell form, 5 the self-collision
// form, 6 the side-memory form, 7 the body self-collision form -- the highest whose trigger an entry of the list sets off (8, the
// attributed form, is set off by the context's switch, below):
//   1  an entry carries a friction coefficient
//   2  an entry with a coefficient has a rigid motion that is not all zero or names a mesh with vertex velocities; or an entry, whatever
//      its own coefficient, names a body surface that has one
//   3  an entry's frame is not the identity, or it is a box
//   4  an entry names an open mesh; 5 ... a sheet that collides with itself; 6 ... a mesh with side memory (sided: this trigger alone,
//      which a higher form does not imply: the latch runs by it); 7 ... a body surface that collides with itself
// own_launch: the collision batches go out in a launch of their own (launch.inc: launch_collision_mesh) instead of as a segment of
// project_multi_kernel or through project_collision_kernel: any mesh registered, named or not, or friction, or a framed entry or a box.
// A mesh that no entry names triggers nothing; neither do the entries from S.n on.
// attribution (admm_hip_enable_contact_attribution; the context's switch, not a property of the list): form 8 whatever the list holds,
// always in a launch of its own; sided keeps its meaning, so the latch still runs by its own trigger.
struct CollisionForm { int form; bool own_launch, sided; };

// facts(id) -> the MeshFacts of mesh id, asked for the meshes the list names only (0 <= id < n_meshes): a caller with records of its
// own builds no table per launch
template <class FactsOf> CollisionForm collision_form_of(const admm_dev::ShapeTable &S, int n_meshes, FactsOf &&facts, bool attribution = false) {
    bool friction = false, moving = false, framed = false, shell = false, self = false, sided = false, bodyself = false;
    for (int q = 0; q < S.n; ++q) {
        const bool mu = S.mu[q] > 0.0;
        friction |= mu;
        framed |= S.framed[q] || S.type[q] == ADMM_SHAPE_BOX;
        if (mu) for (int k = 0; k < 9; ++k) moving |= S.motion[q][k] != 0.0;
        const int id = S.type[q] == ADMM_SHAPE_MESH ? (int)S.par[q][3] : -1;
        if (id < 0 || id >= n_meshes) continue;
        const MeshFacts m = facts(id);
        moving |= (m.body && m.body_mu > 0.0) || (mu && m.has_vel);
        shell |= m.thickness > 0.0;
        self |= m.self_collision;
        sided |= m.side_reach > 0.0;
        bodyself |= m.body_self_r > 0.0;
    }
    const int form = bodyself ? 7 : sided ? 6 : self ? 5 : shell ? 4 : framed ? 3 : moving ? 2 : friction ? 1 : 0;
    if (attribution) return CollisionForm{8, true, sided};
    return CollisionForm{form, n_meshes > 0 || friction || framed, sided};
}

// ---- the device tables beside d_meshes ----------------------------------------------------------------------------------------------
// what the tables depend on in a registered mesh: its owner range [own_first, own_first + own_count) (own_count 0: none; two meshes'
// ranges are equal or disjoint), the caller's node behind every vertex of a body surface (n_body_nodes 0: an obstacle), and the self /
// side fields of MeshFacts with all three body-self lengths
struct MeshPlanInput {
    int own_first, own_count; const int *body_nodes; int n_body_nodes;
    bool self_collision; double body_self[3]; double side_reach;
};

// A table that no mesh needs stays EMPTY: its device pointer stays null, which the kernels read as "feature absent".
struct MeshTables {
    std::vector<int> owner;          // [meshes] the owner group (one per distinct range, numbered in mesh order; -1: no owner)
    std::vector<int> tag;            // [n_nodes], device order: the node's owner group (-1: none); empty when no mesh has an owner
    bool any_sheet_self = false, any_body_self = false;      // does a sheet / a body surface collide with itself?
    std::vector<int> self_flag;      // [meshes] 1: a sheet that collides with itself; empty without one
    std::vector<int> vid;            // [n_nodes], device order: the node's vertex id on the self-colliding surface (sheet or body) that
                                     // holds it (-1: none; the later mesh where two hold it); empty without such a surface
    std::vector<double> body_self;   // [meshes][3] the lengths of the bodies that collide with themselves (zeros: off); empty without one
    std::vector<int> side_row;       // [meshes] the mesh's row of side memory, counted in mesh order (-1: none); always filled
    int n_side_rows = 0;
};

// iperm[caller's node] = its position in device order
inline MeshTables plan_mesh_tables(int n_nodes, const int *iperm, const std::vector<MeshPlanInput> &meshes) {
    MeshTables T;
    const size_t nm = meshes.size();
    std::vector<std::pair<int, int> > groups;
    T.owner.assign(nm, -1);
    T.side_row.assign(nm, -1);
    for (size_t i = 0; i < nm; ++i) {
        const MeshPlanInput &M = meshes[i];
        if (M.side_reach > 0.0) T.side_row[i] = T.n_side_rows++;
        if (M.self_collision) T.any_sheet_self = true; else if (M.body_self[0] > 0.0) T.any_body_self = true;
        if (!M.own_count) continue;
        size_t g = 0;
        while (g < groups.size() && groups[g] != std::make_pair(M.own_first, M.own_count)) ++g;
        if (g == groups.size()) groups.push_back(std::make_pair(M.own_first, M.own_count));
        T.owner[i] = (int)g;
    }
    if (!groups.empty()) {
        T.tag.assign((size_t)n_nodes, -1);
        for (size_t g = 0; g < groups.size(); ++g)
            for (int k = groups[g].first; k < groups[g].first + groups[g].second; ++k) T.tag[iperm[k]] = (int)g;
    }
    if (T.any_sheet_self) T.self_flag.assign(nm, 0);
    if (T.any_sheet_self || T.any_body_self) T.vid.assign((size_t)n_nodes, -1);
    if (T.any_body_self) T.body_self.assign(3 * nm, 0.0);
    for (size_t i = 0; i < nm; ++i) {
        const MeshPlanInput &M = meshes[i];
        const bool body = M.body_self[0] > 0.0;
        if (!M.self_collision && !body) continue;
        if (M.self_collision) T.self_flag[i] = 1;
        if (body && T.any_body_self) for (int j = 0; j < 3; ++j) T.body_self[3 * i + j] = M.body_self[j];
        for (int k = 0; k < M.n_body_nodes; ++k) T.vid[iperm[M.body_nodes[k]]] = k;
    }
    return T;
}

} // namespace admm_lib
