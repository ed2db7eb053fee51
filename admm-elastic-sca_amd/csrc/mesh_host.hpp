// mesh_host.hpp -- a closed triangle mesh prepared for collision queries (admm_hip_mesh of include/admm_hip.h): the flat arrays of
// mesh_query.hpp, built and validated on the host by mesh.cpp, and the topology that admm_hip_mesh_set_vertices / the device update
// (kernels_mesh.hpp) recompute them from.  A context copies all of it at admm_hip_add_collision_mesh and uploads it at finalize.
#pragma once
#include <vector>
#include "mesh_query.hpp"

struct admm_hip_mesh {
    std::vector<admm_mesh::Node> nodes;     // BVH, root first
    std::vector<admm_mesh::Tri> tris;       // leaf order
    std::vector<admm_mesh::Nrm> nrm;        // leaf order
    int depth = 0;                          // levels below the root
    double thickness = 0.0;                 // 0: a closed mesh; > 0: an open surface (admm_hip_mesh_create_open), a shell of this half thickness
    // topology (fixed at creation)
    int nv = 0;
    std::vector<int> cid;                   // [nt][3] canonical corner ids (rotated: lowest id first) by original triangle
    std::vector<int> adj;                   // [nt][3] the triangle across edge k (corners k, k + 1) of original triangle t
    std::vector<int> inc_ptr, inc;          // vertex -> its incidences 3 t + k, ascending
    std::vector<int> lvl_ptr, lvl_nodes;    // BVH nodes grouped by depth: level d = lvl_nodes[lvl_ptr[d], lvl_ptr[d + 1])
    // side memory (mesh_query.hpp): per leaf slot, bit reg (1..6) set where that feature is a boundary edge or a vertex incident to one,
    // in the slot's rotated corner order; all zero for a closed mesh
    std::vector<int> bnd;
};

namespace admm_mesh {
// admm_hip_mesh_set_vertices on a mesh object (a context's copy before finalize too)
int mesh_set_vertices(admm_hip_mesh &M, int nv, const double *verts, char *err, int err_len);
// ADMM_OK, or ADMM_ERR_ARG with the refusal's message (the lowest bad triangle first)
int mesh_refusal(const admm_hip_mesh &M, const double *verts, const UpdateCheck &c, char *err, int err_len);
// a sheet that collides with itself (admm_hip_set_sheet_self_collision): does a vertex lie nearer than the half thickness to a triangle it
// is not a corner of?  The lowest such vertex, its triangle and the distance
bool sheet_rest_violation(const admm_hip_mesh &M, int *vtx, int *tri, double *dist);
// a body surface that collides with itself (admm_hip_set_body_self_collision): would the rule move one of M's own vertices where M stands,
// with the rest shape rest [nv][3]?  The lowest such vertex, the winning triangle and the distance
bool body_rest_violation(const admm_hip_mesh &M, const double *rest, double r, double R, double rho, int *vtx, int *tri, double *dist);
}
