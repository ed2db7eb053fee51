// Two-way contact through the class API: scene_bodies' two bars (a NeoHookean cantilever A and a free bar B dropped across it, each
// a CollisionBody behind a floor) with contact attribution on and reaction shares on both surfaces.
//
//   surface_reaction <in.bin> <out.bin> <frames> <iters> <share A> <share B>
// in.bin : int32 nn, ntet, nanch, na, nta, ntb; double x[nn][3], m[nn]; int32 tets[ntet][4], anch[nanch], trisA[nta][3], trisB[ntb][3];
//          double floor_y, dt.  A is nodes [0, na), B nodes [na, nn).
// out.bin: frames x (3 nn doubles of m_x, 3 nn of m_v, 3 nn of the reaction's dv, then n_contacts and n_reacting as doubles)
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

template <class T> bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: surface_reaction in out frames iters share_a share_b\n"); return 1; }
    const int frames = std::atoi(argv[3]), iters = std::atoi(argv[4]);
    const double share_a = std::atof(argv[5]), share_b = std::atof(argv[6]);
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 4;
    int32_t hdr[6];
    if (!rd(in, hdr, 6)) return 4;
    const int nn = hdr[0], ntet = hdr[1], nanch = hdr[2], na = hdr[3], nta = hdr[4], ntb = hdr[5];
    std::vector<double> x(3 * (size_t)nn), m((size_t)nn), tail(2);
    std::vector<int32_t> tets(4 * (size_t)ntet), anch((size_t)nanch), ta(3 * (size_t)nta), tb(3 * (size_t)ntb);
    if (!rd(in, x.data(), x.size()) || !rd(in, m.data(), m.size()) || !rd(in, tets.data(), tets.size()) || !rd(in, anch.data(), anch.size()) ||
        !rd(in, ta.data(), ta.size()) || !rd(in, tb.data(), tb.size()) || !rd(in, tail.data(), 2)) return 4;
    std::fclose(in);
    System system;
    system.settings.verbose = 0;
    system.settings.timestep_s = tail[1];
    system.settings.admm_iters = iters;
    system.settings.contact_attribution = true;
    Eigen::VectorXd X(3 * nn), M(3 * nn);
    for (int i = 0; i < 3 * nn; ++i) { X[i] = x[i]; M[i] = m[i / 3]; }
    system.add_nodes(X, M);
    for (int t = 0; t < ntet; ++t)
        system.forces.push_back(std::shared_ptr<Force>(new HyperElasticTet(tets[4 * t], tets[4 * t + 1], tets[4 * t + 2], tets[4 * t + 3], 1e5, 1e5, 5, "nh")));
    for (int a = 0; a < nanch; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anch[a])));
    std::shared_ptr<CollisionBody> body_a(new CollisionBody(0, na, std::vector<int>(ta.begin(), ta.end())));
    std::shared_ptr<CollisionBody> body_b(new CollisionBody(na, nn - na, std::vector<int>(tb.begin(), tb.end())));
    body_a->reaction_share = share_a;
    body_b->reaction_share = share_b;
    std::vector<std::shared_ptr<CollisionShape> > shapes;
    shapes.push_back(std::shared_ptr<CollisionShape>(new CollisionFloor(Eigen::Vector3d(0, tail[0], 0))));
    shapes.push_back(body_a);
    shapes.push_back(body_b);
    system.forces.push_back(std::shared_ptr<Force>(new CollisionForce(shapes)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Eigen::Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) { std::fclose(f); return 3; }
        const System::SurfaceReaction r = system.surface_reaction();
        if (!r.ok) { std::fclose(f); return 3; }
        const double counts[2] = {(double)r.info.n_contacts, (double)r.info.n_reacting};
        std::fwrite(system.m_x.data(), sizeof(double), 3 * (size_t)nn, f);
        std::fwrite(system.m_v.data(), sizeof(double), 3 * (size_t)nn, f);
        std::fwrite(r.dv.data(), sizeof(double), 3 * (size_t)nn, f);
        std::fwrite(counts, sizeof(double), 2, f);
    }
    std::fclose(f);
    std::printf("surface_reaction: %d nodes, %d + %d surface triangles, shares %g and %g, %d frames x %d iterations\n", nn, nta, ntb, share_a, share_b, frames, iters);
    return 0;
}
