// A rigid attachment through the class API: rigid.cpp's scene (the two bars, each a CollisionBody behind a floor, and a CollisionSphere
// that is a rigid body under gravity) with the sphere beside bar B and the nodes of bar A's free end fastened to it by MovingAnchors
// whose `body` is the sphere (MovingAnchor::body; admm_hip_attach_anchors), with contact attribution on.
//
//   attachments <in.bin> <out.bin> <frames> <iters>
// in.bin : int32 nn, ntet, nanch, na, nta, ntb, nend; double x[nn][3], m[nn]; int32 tets[ntet][4], anch[nanch], trisA[nta][3],
//          trisB[ntb][3], end[nend]; double floor_y, dt, centre[3], radius, mass, inertia[6], accel[3].  A is nodes [0, na), B [na, nn).
// out.bin: the body's admm_hip_rigid_state after the last frame, then its attachment row: force[3], torque[3] (doubles)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "System.hpp"
#include "TetForce.hpp"
#include "AnchorForce.hpp"
#include "CollisionFloor.hpp"
#include "CollisionSphere.hpp"
#include "CollisionForce.hpp"
#include "ExplicitForce.hpp"

using namespace admm;

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: attachments in out frames iters\n"); return 1; }
    const int frames = std::atoi(argv[3]), iters = std::atoi(argv[4]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 4;
    int32_t hdr[7];
    if (!rd(in, hdr, 7)) return 4;
    const int nn = hdr[0], ntet = hdr[1], nanch = hdr[2], na = hdr[3], nta = hdr[4], ntb = hdr[5], nend = hdr[6];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), tail(16);
    std::vector<int32_t> tets(4 * (size_t)ntet), anch((size_t)nanch), ta(3 * (size_t)nta), tb(3 * (size_t)ntb), end((size_t)nend);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, anch.data(), anch.size()) ||
        !rd(in, ta.data(), ta.size()) || !rd(in, tb.data(), tb.size()) || !rd(in, end.data(), end.size()) || !rd(in, tail.data(), tail.size())) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = tail[1];
    system.settings.admm_iters = iters;
    system.settings.contact_attribution = true;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    std::shared_ptr<CollisionSphere> ball(new CollisionSphere(Eigen::Vector3d(tail[2], tail[3], tail[4]), tail[5]));
    ball->rigid_mass = tail[6];
    for (int j = 0; j < 6; ++j) ball->rigid_inertia[j] = tail[7 + j];
    ball->rigid_accel = Eigen::Vector3d(tail[13], tail[14], tail[15]);
    for (int t = 0; t < ntet; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new HyperElasticTet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3], 1e5, 1e5, 5, "nh")));
    for (int a = 0; a < nanch; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anch[a])));
    std::vector<std::shared_ptr<ControlPoint> > points;
    for (int e = 0; e < nend; ++e) {
        const int id = end[e];
        points.push_back(std::shared_ptr<ControlPoint>(new ControlPoint(Eigen::Vector3d(x[3 * id], x[3 * id + 1], x[3 * id + 2]))));
        std::shared_ptr<MovingAnchor> ma(new MovingAnchor(id, points.back()));
        ma->body = ball;
        system.forces.push_back(ma);
    }
    std::shared_ptr<CollisionBody> body_a(new CollisionBody(0, na, std::vector<int>(ta.begin(), ta.end())));
    std::shared_ptr<CollisionBody> body_b(new CollisionBody(na, nn - na, std::vector<int>(tb.begin(), tb.end())));
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Eigen::Vector3d(0, tail[0], 0))));
    shapes.push_back(body_a);
    shapes.push_back(body_b);
    shapes.push_back(ball);
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    for (int fr = 0; fr < frames; ++fr) if (!system.step()) return 3;
    const std::vector<admm_hip_rigid_state> r = system.rigid_state();
    const std::vector<System::AttachmentLoad> load = system.attachment_load();
    if (r.size() != 1 || load.size() != 1 || !system.attachment_targets()) return 3;
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    std::fwrite(r.data(), sizeof(admm_hip_rigid_state), 1, f);
    std::fwrite(load[0].force, sizeof(double), 3, f);
    std::fwrite(load[0].torque, sizeof(double), 3, f);
    std::fclose(f);
    std::printf("attachments: %d nodes, %d anchors on the sphere, %d frames x %d iterations; the sphere's centre y %.6f, %lld contacts, carried F_y %.4g; first control point y %.6f\n", nn,
                nend, frames, iters, r[0].c[1], (long long)r[0].count, load[0].force[1], points[0]->pos[1]);
    return 0;
}
