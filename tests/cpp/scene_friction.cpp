// A tet slab (LinearTetStrain) lying on a floor under tilted gravity, with Coulomb friction at the floor, through the class API.
//
//   scene_friction <mode> <in.bin> <out.bin> <frames> <iters>
//   mode 0  CollisionForce { CollisionFloor, friction = mu }      the device's friction kernel; m_x after every frame -> out.bin
//   mode 1  CollisionForce { UserFloor, friction = mu }           a user-written shape projects on the host: initialize must refuse
//   mode 2  CollisionForce { CollisionFloor, CollisionBody with friction = mu }   a moving simulated surface: initialize must refuse
// in.bin : int32 nn, ntet, ntri; double x[nn][3], m[nn]; int32 tets[ntet][4], tris[ntri][3] (the slab's surface); double g[3], mu
// out.bin: frames x 3 nn doubles
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

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: scene_friction mode in out frames iters\n"); return 1; }
    const int mode = std::atoi(argv[1]), frames = std::atoi(argv[4]), iters = std::atoi(argv[5]);
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 4;
    int32_t hdr[3];
    if (!rd(in, hdr, 3)) return 4;
    const int nn = hdr[0], ntet = hdr[1], ntri = hdr[2];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), gm(4);
    std::vector<int32_t> tets(4 * (size_t)ntet), tris(3 * (size_t)ntri);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, tris.data(), tris.size()) || !rd(in, gm.data(), 4)) return 4;
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
    const Eigen::Vector3d floor_c(0, 0, 0);
    if (mode == 1) shapes.push_back(std::shared_ptr<CollisionShape>(new UserFloor(floor_c)));
    else shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(floor_c)));
    if (mode != 2) shapes[0]->friction = gm[3];
    if (mode == 2) {
        shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionBody(0, nn, std::vector<int>(tris.begin(), tris.end()))));
        shapes[1]->friction = gm[3];
    }
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(gm[0], gm[1], gm[2]))));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[3], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) { std::fclose(f); return 3; }
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
    }
    std::fclose(f);
    std::printf("scene_friction: mode %d, %d nodes, %d tets, mu %g, %d frames x %d iterations\n", mode, nn, ntet, gm[3], frames, iters);
    return 0;
}
