// Friction against moving obstacles and body surfaces through the class API.
//
//   scene_moving_friction <mode> <in.bin> <out.bin> <frames> <iters>
//   mode 0  a tet slab (LinearTetStrain) on a CollisionMesh platform with friction = inf that the program translates by v dt a frame and
//           whose lin_velocity = v: the slab is carried along
//   mode 1  two such slabs stacked, the lower one's bottom layer anchored, each slab's surface a CollisionBody with surface_friction = mu,
//           under tilted gravity
// in.bin : int32 nn, ntet, ntri, nv, nf; double x[nn][3], m[nn]; int32 tets[ntet][4], tris[ntri][3] (the slab's surface);
//          double verts[nv][3]; int32 faces[nf][3] (the platform); double t0[3], v[3], g[3], mu
// out.bin: frames x (3 x nodes) doubles, m_x after every frame
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
    if (argc < 6) { std::fprintf(stderr, "usage: scene_moving_friction mode in out frames iters\n"); return 1; }
    const int mode = std::atoi(argv[1]), frames = std::atoi(argv[4]), iters = std::atoi(argv[5]);
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 4;
    int32_t hdr[5];
    if (!rd(in, hdr, 5)) return 4;
    const int nn = hdr[0], ntet = hdr[1], ntri = hdr[2], nv = hdr[3], nf = hdr[4];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), verts(3 * (size_t)nv), par(10);
    std::vector<int32_t> tets(4 * (size_t)ntet), tris(3 * (size_t)ntri), faces(3 * (size_t)nf);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, tris.data(), tris.size()) ||
        !rd(in, verts.data(), verts.size()) || !rd(in, faces.data(), faces.size()) || !rd(in, par.data(), 10)) return 4;
    std::fclose(in);
    const Eigen::Vector3d t0(par[0], par[1], par[2]), vb(par[3], par[4], par[5]), g(par[6], par[7], par[8]);
    const double mu = par[9], dt = 0.02;
    const int bodies = mode == 1 ? 2 : 1, total = bodies * nn;
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = dt;
    system.settings.admm_iters = iters;
    Eigen::VectorXd X(3 * total), M(3 * total);
    for (int b = 0; b < bodies; ++b)
        for (int i = 0; i < 3 * nn; ++i) { X[3 * nn * b + i] = x[i] + ((b == 1 && i % 3 == 1) ? 0.1 : 0.0); M[3 * nn * b + i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int b = 0; b < bodies; ++b)
        for (int t = 0; t < ntet; ++t)
            system.forces.push_back(std::shared_ptr<Force>(new LinearTetStrain(tets[4 * t] + b * nn, tets[4 * t + 1] + b * nn, tets[4 * t + 2] + b * nn, tets[4 * t + 3] + b * nn, 2e4)));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    std::shared_ptr<CollisionMesh> platform;
    if (mode == 0) {
        platform = std::shared_ptr<CollisionMesh>(new CollisionMesh(t0, verts, std::vector<int>(faces.begin(), faces.end())));
        platform->friction = INFINITY;
        shapes.push_back(platform);
        system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0.0, -9.8, 0.0))));
    } else {
        for (int i = 0; i < nn; ++i) if (x[3 * i + 1] == 0.0) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(i)));
        for (int b = 0; b < 2; ++b) {
            std::vector<int> t(tris.begin(), tris.end());
            for (size_t i = 0; i < t.size(); ++i) t[i] += b * nn;
            std::shared_ptr<CollisionBody> cb(new CollisionBody(b * nn, nn, t));
            cb->surface_friction = mu;
            shapes.push_back(cb);
        }
        system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(g)));
    }
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[3], "wb");
    if (!f) return 4;
    Eigen::Vector3d t = t0;
    for (int fr = 0; fr < frames; ++fr) {
        if (mode == 0) {
            for (int j = 0; j < 3; ++j) t[j] = t[j] + dt * vb[j];
            platform->center = t;
            platform->lin_velocity = vb;
        }
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)total, f);
    }
    std::fclose(f);
    std::printf("scene_moving_friction: mode %d, %d nodes, %d frames x %d iterations\n", mode, total, frames, iters);
    return 0;
}
