// A Neo-Hookean bar through the class API with Anderson acceleration switched on from the command line (Settings::parse_args: -aa),
// for the test that reproduces its x bit for bit on the Python path (tests/test_anderson.py).
// usage: scene_anderson <in.bin> <out.bin> <frames> -it <iters> -aa <window> -v 0
//   in.bin : int32 n_nodes, n_tets, n_anchor, type(0 nh / 1 stvk); f64 x[3n], m[3n]; int32 tets[4*n_tets]; int32 anchors[n_anchor]
//   out.bin: f64 x[3n] after every frame
//   stdout : one line per ADMM iteration of the last frame: "iter <accepted> <m_used> <extrapolated> <rho as %a>"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "admm/System.hpp"
using namespace admm;

int main(int argc, char **argv) {
    if (argc < 4) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int hdr[4];
    if (fread(hdr, sizeof(int), 4, f) != 4) return 1;
    const int n = hdr[0], nt = hdr[1], na = hdr[2], type = hdr[3];
    std::vector<double> x(3 * n), m(3 * n); std::vector<int> tets(4 * nt), anchors(na);
    if (fread(x.data(), 8, 3 * n, f) != (size_t)3 * n || fread(m.data(), 8, 3 * n, f) != (size_t)3 * n) return 1;
    if (fread(tets.data(), 4, 4 * nt, f) != (size_t)4 * nt || fread(anchors.data(), 4, na, f) != (size_t)na) return 1;
    fclose(f);
    const int frames = atoi(argv[3]);

    System system;
    system.settings.timestep_s = 0.04;
    system.settings.parse_args(argc - 3, argv + 3);      // (argv[3] stands where the program name would: -it, -aa, -v follow it)
    VectorXd xv(3 * n), mv(3 * n);
    for (int i = 0; i < 3 * n; ++i) { xv[i] = x[i]; mv[i] = m[i]; }
    system.add_nodes(xv, mv);
    for (int e = 0; e < nt; ++e)
        system.forces.push_back(std::shared_ptr<Force>(new HyperElasticTet(tets[4 * e], tets[4 * e + 1], tets[4 * e + 2], tets[4 * e + 3], 1e5, 1e5, 5, type ? "stvk" : "nh")));
    for (int a = 0; a < na; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(anchors[a])));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    if (!system.initialize()) return 2;

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;
    for (int fr = 0; fr < frames; ++fr) {
        if (!system.step()) return 3;
        fwrite(system.m_x.data(), 8, 3 * n, o);
    }
    fclose(o);
    const std::vector<admm_hip_acceleration_record> log = system.acceleration_log();
    for (size_t k = 0; k < log.size(); ++k) printf("iter %d %d %d %a\n", (int)log[k].accepted, (int)log[k].m_used, (int)log[k].extrapolated, log[k].rho);
    return 0;
}
