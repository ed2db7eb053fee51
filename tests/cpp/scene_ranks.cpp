// One admm::System per rank through the class API (System::shard): the scene of scene_bar.cpp -- HyperElasticTet bar or a
// cloth-like spring/anchor set-up is not needed here: NH / StVK tets, StaticAnchors, a scripted MovingAnchor that is released
// at frame 3, gravity -- run by `world` ranks that each build the whole System and own a shard of the elements.  A process
// hosts one rank, or several (one host thread and one System each: a comma-separated rank list), so that a wide world
// needs fewer processes on one GPU.
// Transport: comm::ShmAllReduce (host memory, one node), so that the ranks can share one GPU in the tests; on a multi-GPU
// node leave shm_name empty and the ranks meet through RCCL (System::shard.rccl_id_file, from the launcher's environment).
// usage: scene_ranks <in.bin> <out.bin[,out.bin...]> <frames> <iters> <rank[,rank...]> <world> <mode 0 contiguous / 1 subtree> [shm_name]
//   in.bin as scene_bar; out.bin (one per listed rank): f64 x[3n] after every frame, then the control point (3)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include "admm/System.hpp"
using namespace admm;

struct Scene {
    int n = 0, nt = 0, na = 0, type = 0, moving = -1;
    std::vector<double> x, m; std::vector<int> tets, anchors;
};

static std::vector<std::string> split(const std::string &s) {
    std::vector<std::string> out; std::stringstream ss(s); std::string item;
    while (std::getline(ss, item, ',')) out.push_back(item);
    return out;
}

static int run_rank(const Scene &sc, const char *out_path, int frames, int iters, int rank, int world, int mode, const char *shm_name) {
    const int n = sc.n;
    const std::vector<double> &x = sc.x;
    System system;
    system.settings.verbose = 0; system.settings.timestep_s = 0.04; system.settings.admm_iters = iters;
    comm::ShmAllReduce shm;
    if (world > 1) {
        system.shard.rank = rank; system.shard.world = world; system.shard.mode = mode ? ADMM_SHARD_SUBTREE : ADMM_SHARD_CONTIGUOUS;
        if (shm_name && shm_name[0]) {
            if (!shm.open(shm_name, rank, world, 1 << 16, 60.0)) { fprintf(stderr, "rank %d: shared-memory segment %s unavailable\n", rank, shm_name); return 4; }
            system.shard.host_allreduce = &comm::ShmAllReduce::hook; system.shard.host_allreduce_user = &shm;
        } else {
            const int local = system.shard.from_env();       // RCCL: id file from the launcher's environment
            if (local >= 0) system.device_id = local;
        }
    }
    VectorXd xv(3 * n), mv(3 * n);
    for (int i = 0; i < 3 * n; ++i) { xv[i] = x[i]; mv[i] = sc.m[i]; }
    system.add_nodes(xv, mv);
    const std::vector<int> &tets = sc.tets;
    for (int e = 0; e < sc.nt; ++e)
        system.forces.push_back(std::shared_ptr<Force>(new HyperElasticTet(tets[4 * e], tets[4 * e + 1], tets[4 * e + 2], tets[4 * e + 3], 1e5, 1e5, 5, sc.type ? "stvk" : "nh")));
    for (int a = 0; a < sc.na; ++a) system.forces.push_back(std::shared_ptr<Force>(new StaticAnchor(sc.anchors[a])));
    const int moving = sc.moving;
    std::shared_ptr<ControlPoint> cp(new ControlPoint(Vector3d(x[3 * moving], x[3 * moving + 1], x[3 * moving + 2])));
    const Vector3d start = cp->pos, end = cp->pos + Vector3d(0.0, 0.05, 0.0);
    system.forces.push_back(std::shared_ptr<Force>(new MovingAnchor(moving, cp)));
    system.explicit_forces.push_back(std::shared_ptr<ExplicitForce>(new ExplicitForce(Vector3d(0, -9.8, 0))));
    system.pre_step_callbacks.push_back([cp, start, end](System *s) { cp->pos = helper::smooth_move(s->elapsed_s, 0.0, 0.2, start, end); });
    if (!system.initialize()) return 2;

    FILE *o = fopen(out_path, "wb");
    if (!o) return 1;
    for (int fr = 0; fr < frames; ++fr) {
        if (fr == 3) cp->active = false;   // release: the control point now follows the node
        if (!system.step()) { fclose(o); return 3; }
        fwrite(system.m_x.data(), 8, 3 * n, o);
    }
    double cpv[3] = {cp->pos[0], cp->pos[1], cp->pos[2]};
    fwrite(cpv, 8, 3, o);
    fclose(o);
    printf("ok rank %d of %d: %d nodes %d forces elapsed %.2f\n", rank, world, n, (int)system.forces.size(), system.elapsed_s);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 8) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int hdr[4];
    if (fread(hdr, sizeof(int), 4, f) != 4) return 1;
    Scene sc;
    sc.n = hdr[0]; sc.nt = hdr[1]; sc.na = hdr[2]; sc.type = hdr[3];
    sc.x.resize(3 * sc.n); sc.m.resize(3 * sc.n); sc.tets.resize(4 * sc.nt); sc.anchors.resize(sc.na);
    if (fread(sc.x.data(), 8, 3 * sc.n, f) != (size_t)3 * sc.n || fread(sc.m.data(), 8, 3 * sc.n, f) != (size_t)3 * sc.n) return 1;
    if (fread(sc.tets.data(), 4, 4 * sc.nt, f) != (size_t)4 * sc.nt || fread(sc.anchors.data(), 4, sc.na, f) != (size_t)sc.na || fread(&sc.moving, 4, 1, f) != 1) return 1;
    fclose(f);
    const int frames = atoi(argv[3]), iters = atoi(argv[4]), world = atoi(argv[6]), mode = atoi(argv[7]);
    const char *shm_name = argc > 8 ? argv[8] : nullptr;
    const std::vector<std::string> outs = split(argv[2]), ranks = split(argv[5]);
    if (outs.empty() || outs.size() != ranks.size()) return 1;

    std::vector<int> rc(ranks.size(), 0);
    if (ranks.size() == 1) {
        rc[0] = run_rank(sc, outs[0].c_str(), frames, iters, atoi(ranks[0].c_str()), world, mode, shm_name);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 0; k < ranks.size(); ++k)
            th.emplace_back([&, k]() { rc[k] = run_rank(sc, outs[k].c_str(), frames, iters, atoi(ranks[k].c_str()), world, mode, shm_name); });
        for (std::thread &t : th) t.join();
    }
    for (int r : rc) if (r != 0) return r;
    return 0;
}
