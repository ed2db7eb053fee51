// A small tet block (LinearTetStrain) falling onto a CollisionBox turned about its centre and a CollisionCylinder with an orientation,
// both in one CollisionForce, through the class API.
//
//   scene_frames <in.bin> <out.bin> <frames> <iters>
// in.bin : int32 nn, ntet; double x[nn][3], m[nn]; int32 tets[ntet][4];
//          double box centre[3], half[3], R[9]; cylinder centre[3], radius, R[9], pivot[3]; the box's friction coefficient
// out.bin: frames x 3 nn doubles (m_x after every frame)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "System.hpp"
#include "TetForce.hpp"
#include "CollisionCylinder.hpp"
#include "CollisionForce.hpp"
#include "ExplicitForce.hpp"

using namespace admm;

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: scene_frames in out frames iters\n"); return 1; }
    const int frames = std::atoi(argv[3]), iters = std::atoi(argv[4]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 4;
    int32_t hdr[2];
    if (!rd(in, hdr, 2)) return 4;
    const int nn = hdr[0], ntet = hdr[1];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), g(32);
    std::vector<int32_t> tets(4 * (size_t)ntet);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, g.data(), 32)) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = 0.02;
    system.settings.admm_iters = iters;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int t = 0; t < ntet; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new LinearTetStrain(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3], 2e4)));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    std::shared_ptr<CollisionBox> box(new CollisionBox(Eigen::Vector3d(g[0], g[1], g[2]), Eigen::Vector3d(g[3], g[4], g[5])));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) box->orientation[i][j] = g[6 + 3 * i + j];
    box->friction = g[31];
    std::shared_ptr<CollisionCylinder> cyl(new CollisionCylinder(Eigen::Vector3d(g[15], g[16], g[17]), Eigen::Vector3d(1, 1, 1), g[18]));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) cyl->orientation[i][j] = g[19 + 3 * i + j];
    cyl->orientation_pivot = Eigen::Vector3d(g[28], g[29], g[30]);
    shapes.push_back(box);
    shapes.push_back(cyl);
    // the box's host evaluation runs the library's rule: its centre is inside and is moved, a far point is not
    if (!(box->isColliding(box->center) > 0) || box->isColliding(Eigen::Vector3d(g[0] + 10, g[1], g[2])) > 0) return 5;
    const Eigen::Vector3d out = box->projectOut(box->center);
    if ((out - box->center).norm() <= 0.0) return 5;
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
    }
    std::fclose(f);
    std::printf("scene_frames: %d nodes, %d tets, %d frames x %d iterations\n", nn, ntet, frames, iters);
    return 0;
}
