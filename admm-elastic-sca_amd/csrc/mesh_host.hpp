// mesh_host.hpp -- a closed triangle mesh prepared for collision queries (admm_hip_mesh of include/admm_hip.h): the flat arrays of
// mesh_query.hpp, built and validated on the host by mesh.cpp.  A context copies them at admm_hip_add_collision_mesh and uploads
// them at finalize.
#pragma once
#include <vector>
#include "mesh_query.hpp"

struct admm_hip_mesh {
    std::vector<admm_mesh::Node> nodes;     // BVH, root first
    std::vector<admm_mesh::Tri> tris;       // leaf order
    std::vector<admm_mesh::Nrm> nrm;        // leaf order
    int depth = 0;                          // levels below the root
};
