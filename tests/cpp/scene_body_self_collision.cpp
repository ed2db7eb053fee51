// A tet body that collides with itself (CollisionBody::self_collision) through the class API: every node belongs to the body, which is
// LinearTetStrain with StaticAnchors; the one CollisionForce's list holds the body's own surface alone.
//
//   scene_body_self_collision <in.bin> <out.bin> <frames> <iters>
// in.bin : int32 nn, ntet, nanch, ntri; double x[nn][3], m[nn]; int32 tets[ntet][4], anch[nanch], tris[ntri][3];
//          double stiffness, gravity, dt, surface_friction, r, reach, rest_radius.
// out.bin: frames x (3 nn doubles of m_x, then 3 nn of m_v) after every frame
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "System.hpp"
#include "TetForce.hpp"
#include "AnchorForce.hpp"
#include "CollisionForce.hpp"
#include "ExplicitForce.hpp"

using namespace admm;

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: scene_body_self_collision in out frames iters\n"); return 1; }
    const int frames = std::atoi(argv[3]), iters = std::atoi(argv[4]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 4;
    int32_t hdr[4];
    if (!rd(in, hdr, 4)) return 4;
    const int nn = hdr[0], ntet = hdr[1], nanch = hdr[2], ntri = hdr[3];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), tail(7);
    std::vector<int32_t> tets(4 * (size_t)ntet), anch((size_t)nanch), tris(3 * (size_t)ntri);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, anch.data(), anch.size()) ||
        !rd(in, tris.data(), tris.size()) || !rd(in, tail.data(), 7)) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = tail[2];
    system.settings.admm_iters = iters;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int t = 0; t < ntet; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new LinearTetStrain(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3], tail[0])));
    for (int a = 0; a < nanch; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anch[a])));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    std::shared_ptr<CollisionBody> body(new CollisionBody(0, nn, std::vector<int>(tris.begin(), tris.end())));
    body->surface_friction = tail[3];
    for (int j = 0; j < 3; ++j) body->self_collision[j] = tail[4 + j];
    shapes.push_back(body);
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -tail[1], 0))));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
        std::fwrite(system.m_v.data(), sizeof(double), 3 * (size_t)nn, f);
    }
    std::fclose(f);
    std::printf("scene_body_self_collision: %d nodes, %d tets, %d surface triangles, %d frames x %d iterations\n", nn, ntet, ntri, frames, iters);
    return 0;
}
