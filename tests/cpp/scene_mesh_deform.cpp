// A tet plate (LinearTetStrain) dropped onto a closed triangle-mesh obstacle that deforms between frames, through the class API:
// before frame f the obstacle's vertices become the creation vertices scaled by 1 + 0.004 f and turned 3f degrees about y
// (CollisionMesh::set_vertices; System::step hands the new shape to its context).
//
//   scene_mesh_deform <mode> <in.bin> <out.bin> <frames> <iters>
//   mode 0  CollisionForce { CollisionFloor }               built-in floor (device)           -- the control pair:
//   mode 1  CollisionForce { UserFloor }                    CollisionFloor's arithmetic as user code (host-projected)
//   mode 2  CollisionForce { CollisionFloor, CollisionMesh } the deforming mesh on the device  -- the mesh pair:
//   mode 3  CollisionForce { CollisionFloor, HostMesh }      a subclass deforming its own host mesh: host-projected, the same query code
//   mode 4  as mode 2, the mesh never deformed
// in.bin : int32 nv, nt, nn, ntet; double verts[nv][3]; int32 tris[nt][3]; double x[nn][3], m[nn]; int32 tets[ntet][4]; double c0[3], rise
//          (the obstacle stays at c0: `rise` is not used here)
// out.bin: frames x 3 nn doubles (m_x after every frame)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "System.hpp"
#include "TetForce.hpp"
#include "CollisionFloor.hpp"
#include "CollisionForce.hpp"
#include "ExplicitForce.hpp"

using namespace admm;

class UserFloor : public CollisionShape {
public:
    UserFloor(Eigen::Vector3d c) : CollisionShape(c) {}
    double isColliding(Eigen::Vector3d pos) const { return center[1] - pos[1]; }
    Eigen::Vector3d projectOut(const Eigen::Vector3d currPos) const { return Eigen::Vector3d(currPos[0], center[1], currPos[2]); }
};

class HostMesh : public CollisionMesh {
public:
    HostMesh(Eigen::Vector3d c, const std::vector<double> &v, const std::vector<int> &t) : CollisionMesh(c, v, t) {}
};

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: scene_mesh_deform mode in out frames iters\n"); return 1; }
    const int mode = std::atoi(argv[1]), frames = std::atoi(argv[4]), iters = std::atoi(argv[5]);
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 4;
    int32_t hdr[4];
    if (!rd(in, hdr, 4)) return 4;
    const int nv = hdr[0], nt = hdr[1], nn = hdr[2], ntet = hdr[3];
    std::vector<double> verts(3 * (size_t)nv), x(3 * (size_t)nn), m((size_t)nn), c0(4);
    std::vector<int32_t> tris(3 * (size_t)nt), tets(4 * (size_t)ntet);
    if (!rd(in, verts.data(), verts.size()) || !rd(in, tris.data(), tris.size()) || !rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) ||
        !rd(in, tets.data(), tets.size()) || !rd(in, c0.data(), 4)) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = 0.02;
    system.settings.admm_iters = iters;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int t = 0; t < ntet; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new LinearTetStrain(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3], 5e3)));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    const Eigen::Vector3d floor_c(0, -2.0, 0);
    if (mode == 1) shapes.push_back(std::shared_ptr<CollisionShape>(new UserFloor(floor_c)));
    else shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(floor_c)));
    const std::vector<int> tri_v(tris.begin(), tris.end());
    std::shared_ptr<CollisionShape> obstacle;
    try {
        if (mode == 2 || mode == 4) obstacle.reset(new CollisionMesh(Eigen::Vector3d(c0[0], c0[1], c0[2]), verts, tri_v));
        if (mode == 3) obstacle.reset(new HostMesh(Eigen::Vector3d(c0[0], c0[1], c0[2]), verts, tri_v));
    } catch (const std::exception &e) { std::fprintf(stderr, "%s\n", e.what()); return 5; }
    if (obstacle) shapes.push_back(obstacle);
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[3], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (obstacle && mode != 4) {      // a deforming obstacle
            CollisionMesh &cm = static_cast<CollisionMesh &>(*obstacle);
            const double a = 3.0 * M_PI / 180.0 * fr, s = 1.0 + 0.004 * fr, ca = std::cos(a), sa = std::sin(a);
            std::vector<double> w(verts.size());
            for (int v = 0; v < nv; ++v) {
                const double px = s * verts[3 * v], py = s * verts[3 * v + 1], pz = s * verts[3 * v + 2];
                w[3 * v] = ca * px + sa * pz; w[3 * v + 1] = py; w[3 * v + 2] = -sa * px + ca * pz;
            }
            try { cm.set_vertices(w); } catch (const std::exception &e) { std::fprintf(stderr, "%s\n", e.what()); std::fclose(f); return 5; }
        }
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
    }
    std::fclose(f);
    std::printf("scene_mesh_deform: mode %d, %d nodes, %d tets, %d mesh triangles, %d frames x %d iterations\n", mode, nn, ntet, nt, frames, iters);
    return 0;
}
