// System.hpp -- host-side mirror of admm::System
// (deps/admm-elastic-sca/src/system/System.hpp:29-76, System.cpp) over the C ABI
// of libadmm_hip.so.  Same public members and methods:
//   settings{timestep_s, verbose, admm_iters} (+ parse_args/help), elapsed_s,
//   m_x, m_v, m_masses, explicit_forces, forces, add_nodes, initialize, step,
//   recompute_weights, pre_step_callbacks.
// initialize() hands nodes and forces to the library (batches of consecutive
// forces of one kind, in forces[] order), step() runs one frame on the GPU and
// leaves m_x / m_v valid on return, like the reference.  There is no CPU path
// for the built-in forces: without a GPU initialize() prints the library's error
// and returns false.
//
// User-written plug-ins keep working (the reference's extension story,
// Force.hpp:37-57 and samples/singletet.cpp:100-102): a Force subclass is asked
// for its selector rows once (get_selector, System.cpp:121-124); every ADMM
// iteration the device evaluates D_i x for those rows, project() runs here on the
// host (System.cpp:57-58) and z - u returns to the device-side right-hand side.
// A user-written ExplicitForce::project runs here at the start of step().
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "Comm.hpp"
#include "Force.hpp"
#include "admm_hip.h"

namespace admm {

class System {
public:
    System() : elapsed_s(0.0), device_id(0), initialized(false), gpu(nullptr), user_rows(0), pinned_x(nullptr), pinned_v(nullptr), seen_x(nullptr), seen_v(nullptr), pinned_bytes(0), init_count(0) {}
    ~System() { release(); }
    System(const System &) = delete;
    System &operator=(const System &) = delete;

    struct Settings {
        void parse_args(int argc, char **argv) {   // System.cpp:182-198
            for (int i = 1; i < argc - 1; ++i) {
                std::string arg(argv[i]);
                std::stringstream val(argv[i + 1]);
                if (arg == "-help") help();
                else if (arg == "-dt") val >> timestep_s;
                else if (arg == "-v") val >> verbose;
                else if (arg == "-it") val >> admm_iters;
                else if (arg == "-aa") val >> anderson_window;
            }
            if (argc > 0) { std::string arg(argv[argc - 1]); if (arg == "-help") help(); }
        }
        void help() {                               // System.cpp:200-208
            printf("\n==========================================\nArgs:\n\t-dt: time step (s)\n\t-v: verbosity (higher -> show more)\n\t-it: # admm iters\n\t-aa: Anderson acceleration window (0 = off)\n==========================================\n");
        }
        double timestep_s;
        int verbose;
        int admm_iters;
        // extension (the reference only describes it, System.cpp:64-65): with residual_tol_primal > 0 a step's ADMM loop
        // ends once |W(Dx-z)| <= residual_tol_primal and |D^T W^T W (z-z_prev)| <= residual_tol_dual, tested every
        // residual_check_every iterations; admm_iters stays the upper bound.  0 (default) = the reference's fixed count.
        double residual_tol_primal, residual_tol_dual;
        int residual_check_every;
        // extension, no reference counterpart: every ADMM iteration of step() records inertia(x_k) and elastic(x_k) of the incremental
        // potential (System::objective(); admm_hip_enable_objective).  Not available on a sharded system.
        bool track_objective;
        // extension, no reference counterpart: Anderson acceleration of the ADMM iteration with a history of that many iterations
        // (0 .. 8; admm_hip_set_acceleration, System::acceleration_log()).  0 (default) = the reference's iteration.  Not available on
        // a sharded system or with user-defined forces.
        int anderson_window;
        // extension, no reference counterpart: every collision element records, in every local step, the entry of its CollisionForce's
        // shape list that last moved it and the direction of that push (admm_hip_enable_contact_attribution; System::contact_owners(),
        // System::entry_resultants()).  false (default): nothing is recorded and nothing else is launched.
        bool contact_attribution;
        Settings() : timestep_s(0.04), verbose(1), admm_iters(10), residual_tol_primal(0.0), residual_tol_dual(0.0), residual_check_every(1), track_objective(false), anderson_window(0),
                     contact_attribution(false) {}
    } settings;

    double elapsed_s;
    VectorXd m_x, m_v, m_masses;   // xyz-interleaved, 3 per node
    std::vector<std::shared_ptr<ExplicitForce> > explicit_forces;
    std::vector<std::shared_ptr<Force> > forces;
    std::vector<std::function<void(System *)> > pre_step_callbacks;
    int device_id;                 // HIP device of this System (one process per GPU)

    // Multi-GPU (no reference counterpart: the reference's element loop, System.cpp:57-58, is one OpenMP team).  One process
    // per GPU, every process builds the SAME System (all nodes, all forces, same order) and sets its rank before initialize():
    // the elements shard across the ranks, the partial right-hand sides meet in one (distributed top: two) small all-reduce(s) per ADMM
    // iteration inside the library, and m_x / m_v are complete on every rank after every step().  Pre-step callbacks, control points and
    // recompute_weights() must run identically on all ranks; under subtree shards initialize() and recompute_weights() are COLLECTIVE calls
    // (every rank factors only its own elimination subtrees + its part of the top; the subtree roots' update matrices meet in one all-reduce).
    struct Shard {
        int rank, world;
        int mode;                        // ADMM_SHARD_SUBTREE (default: ranks own elimination subtrees, small exchange) or ADMM_SHARD_CONTIGUOUS
        bool factor_local;               // subtree shards: every rank factors and keeps its own share (default; false: the whole matrix on every rank, initialize() stays local)
        // RCCL (default transport): rank 0 publishes the communicator's 128-byte id in this file, the others wait for it
        // (Comm.hpp rccl_id_via_file; a path unique to the job, on a filesystem all ranks see)
        std::string rccl_id_file;
        double rendezvous_timeout_s, rendezvous_max_age_s;
        // any other transport instead: a hook that sums a DEVICE buffer (admm_hip_set_allreduce) or a HOST buffer
        // (admm_hip_set_host_allreduce, e.g. comm::ShmAllReduce::hook) in place across the ranks
        admm_hip_allreduce_fn allreduce; void *allreduce_user;
        admm_hip_host_allreduce_fn host_allreduce; void *host_allreduce_user;
        Shard() : rank(0), world(1), mode(ADMM_SHARD_SUBTREE), factor_local(true), rendezvous_timeout_s(600.0), rendezvous_max_age_s(600.0),
                  allreduce(nullptr), allreduce_user(nullptr), host_allreduce(nullptr), host_allreduce_user(nullptr) {}
        // what a launcher exports: torchrun / torch.distributed.run (RANK, WORLD_SIZE, LOCAL_RANK), Open MPI, Slurm;
        // ADMM_HIP_RCCL_ID_FILE names the rendezvous file.  Returns the local rank (the caller's device_id), or -1 if no launcher is seen.
        int from_env() {
            static const char *const rk[] = {"RANK", "OMPI_COMM_WORLD_RANK", "SLURM_PROCID"}, *const wd[] = {"WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", "SLURM_NTASKS"},
                              *const lr[] = {"LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID"};
            for (int i = 0; i < 3; ++i) {
                const char *r = std::getenv(rk[i]), *w = std::getenv(wd[i]), *l = std::getenv(lr[i]);
                if (!r || !w) continue;
                rank = std::atoi(r); world = std::atoi(w);
                if (const char *f = std::getenv("ADMM_HIP_RCCL_ID_FILE")) rccl_id_file = f;
                else if (rccl_id_file.empty()) {
                    // per launch: the launcher's rendezvous port / job id tells two jobs on one node apart (and Comm.hpp's launch_nonce(), stored in the
                    // file, a crashed earlier launch's leftover).  Nothing job-unique in the environment: the name stays empty and initialize()
                    // fails with a message that asks for ADMM_HIP_RCCL_ID_FILE -- never a name two jobs could share.
                    const char *tag = std::getenv("MASTER_PORT"); if (!tag) tag = std::getenv("SLURM_JOB_ID"); if (!tag) tag = std::getenv("OMPI_MCA_ess_base_jobid");
                    if (!tag) tag = std::getenv("PMIX_NAMESPACE");
                    if (tag) rccl_id_file = std::string("/tmp/admm_hip_rccl_id.") + std::to_string((long)getuid()) + "." + tag;
                }
                return l ? std::atoi(l) : rank;
            }
            return -1;
        }
    } shard;

    // System.cpp:78-95
    int add_nodes(VectorXd x, VectorXd m) {
        const int old_n = (int)m_x.size(), add = (int)x.size();
        unpin_state();             // the vectors are about to be re-allocated: never leave a freed buffer page-locked
        m_x.conservativeResize(old_n + add); m_v.conservativeResize(old_n + add); m_masses.conservativeResize(old_n + add);
        for (int i = 0; i < add; ++i) { m_x[old_n + i] = x[i]; m_v[old_n + i] = 0.0; m_masses[old_n + i] = m[i]; }
        return (old_n + add) / 3;
    }

    // System.cpp:98-156
    bool initialize() {
        const int dof = (int)m_x.size();
        if (settings.verbose > 0) std::cout << "Solver::initialize: " << std::endl;
        if (settings.timestep_s <= 0.0) {
            std::cerr << "\n**Solver Error: timestep set to " << settings.timestep_s << "s, changing to 0.04s." << std::endl;
            settings.timestep_s = 0.04;
        }
        if (!(m_masses.size() == m_x.size() && m_x.size() >= 3)) { std::cerr << "\n**Solver Error: Problem with node data!" << std::endl; return false; }
        release();                  // (also un-pins m_x / m_v before they may be re-allocated)
        // an UNCHANGED scene binary under a launcher: ADMM_HIP_RANKS_FROM_ENV=1 makes every process take its rank, world size
        // and GPU from the launcher's environment (mpirun -np 8 -x ADMM_HIP_RANKS_FROM_ENV=1 ./windyflag)
        if (shard.world == 1) { const char *auto_env = std::getenv("ADMM_HIP_RANKS_FROM_ENV"); if (auto_env && std::atoi(auto_env) != 0) { const int local = shard.from_env(); if (local >= 0) device_id = local; } }
        if (m_v.size() < m_x.size()) m_v.resize(m_x.size());
        m_v.setZero();
        if (admm_hip_create(&gpu, device_id) != ADMM_OK) { std::cerr << "\n**Solver Error: no usable HIP device " << device_id << " (the built-in forces have no CPU path)" << std::endl; gpu = nullptr; return false; }
        if (!check(admm_hip_set_timestep(gpu, settings.timestep_s))) return false;
        if (!check(admm_hip_keep_z(gpu, 0))) return false;       // curr_z is not part of the class's public surface: no need to store it every iteration
        if (!setup_shard()) return false;
        if (!check(admm_hip_add_nodes(gpu, dof / 3, m_x.data(), m_masses.data(), nullptr))) return false;
        // Force::initialize of the user-written forces (System.cpp:117-119); the built-in ones compute their rest data in the library
        for (size_t i = 0; i < forces.size(); ++i) {
            Force &f = *forces[i];
            if (f.kind() >= 0 && typeid(f) != f.device_type()) {
                std::cerr << "\n**Solver Error: force " << i << " derives from a built-in force class; a subclass must override kind() to return -1 and bring its own get_selector()/project()" << std::endl;
                return false;
            }
            if (const CollisionForce *cf = dynamic_cast<const CollisionForce *>(&f))      // friction is applied by the device's collision kernel only
                for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
                    const CollisionShape &sh = *cf->collisionShapes[q];
                    if (sh.friction == 0.0) continue;
                    if (f.kind() < 0) {
                        std::cerr << "\n**Solver Error: force " << i << ", shape " << q << ": friction " << sh.friction << " on a force that projects on the host (a user-written shape in its list); friction needs the device form of every shape" << std::endl;
                        return false;
                    }
                    if (dynamic_cast<const CollisionBody *>(&sh)) {
                        std::cerr << "\n**Solver Error: force " << i << ", shape " << q << ": friction " << sh.friction << " on a CollisionBody; contact with a moving simulated surface takes no friction" << std::endl;
                        return false;
                    }
                }
            if (f.kind() < 0) {
                if (const CollisionForce *cf = dynamic_cast<const CollisionForce *>(&f))      // a built-in shape's orientation is applied by the device only (CollisionBox applies its own)
                    for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
                        const CollisionShape &sh = *cf->collisionShapes[q];
                        bool turned = false;
                        for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) turned = turned || sh.orientation[a][c] != (a == c ? 1.0 : 0.0);
                        if (turned && !dynamic_cast<const CollisionBox *>(&sh)) {
                            std::cerr << "\n**Solver Error: force " << i << ", shape " << q << ": an orientation on a force that projects on the host (a user-written shape in its list); it needs the device form of every shape" << std::endl;
                            return false;
                        }
                    }
                if (const CollisionForce *cf = dynamic_cast<const CollisionForce *>(&f))      // side memory lives in the context: the device form only, like an orientation
                    for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
                        const CollisionMesh *cm = dynamic_cast<const CollisionMesh *>(cf->collisionShapes[q].get());
                        if (cm && cm->side_reach != 0.0) {
                            std::cerr << "\n**Solver Error: force " << i << ", shape " << q << ": side memory (side_reach " << cm->side_reach << ") on a force that projects on the host (a user-written shape in its list); it needs the device form of every shape" << std::endl;
                            return false;
                        }
                    }
                if (const CollisionForce *cf = dynamic_cast<const CollisionForce *>(&f))      // body self-collision runs in the device form only, like an orientation
                    for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
                        const CollisionBody *cb = dynamic_cast<const CollisionBody *>(cf->collisionShapes[q].get());
                        if (cb && !dynamic_cast<const CollisionSheet *>(cb) && cb->self_collision[0] != 0.0) {
                            std::cerr << "\n**Solver Error: force " << i << ", shape " << q << ": body self-collision (r " << cb->self_collision[0] << ") on a force that projects on the host (a user-written shape in its list); it needs the device form of every shape" << std::endl;
                            return false;
                        }
                    }
                if (const CollisionForce *cf = dynamic_cast<const CollisionForce *>(&f))
                    for (size_t q = 0; q < cf->collisionShapes.size(); ++q) if (dynamic_cast<const CollisionBody *>(cf->collisionShapes[q].get())) {
                        std::cerr << "\n**Solver Error: force " << i << " projects on the host (a user-written shape in its list), where a CollisionBody has no evaluation" << std::endl;
                        return false;
                    }
                f.initialize(m_x, m_v, m_masses, settings.timestep_s);
            }
        }
        // consecutive forces of one kind (and one anchor flavour) -> one batch, order preserved
        batch_first.clear(); batch_count.clear(); batch_kind.clear(); batch_moving.clear(); batch_urow0.clear(); batch_body.clear();
        user_rows = 0;
        std::vector<double> user_weights;
        for (size_t i = 0; i < forces.size();) {
            const int kind = forces[i]->kind();
            if (kind < 0) {      // a run of user-written forces -> one generic batch
                std::vector<Eigen::Triplet<double> > trips;
                const size_t row0 = user_weights.size();
                std::vector<int32_t> erp(1, 0);
                size_t j = i;
                for (; j < forces.size() && forces[j]->kind() < 0; ++j) {
                    const size_t w0 = user_weights.size(), t0 = trips.size();
                    forces[j]->get_selector(m_x, trips, user_weights);
                    for (size_t t = t0; t < trips.size(); ++t) if (trips[t].row() < (long)w0 || trips[t].row() >= (long)user_weights.size() || trips[t].col() < 0 || trips[t].col() >= dof) {
                        std::cerr << "\n**Solver Error: force " << j << " pushed a selector triplet (row " << trips[t].row() << ", col " << trips[t].col() << ") outside the rows [" << w0 << ", " << user_weights.size() << ") it announced through weights" << std::endl;
                        return false;
                    }
                    erp.push_back((int32_t)(user_weights.size() - row0));
                }
                std::vector<int32_t> tr(trips.size()), tc(trips.size()); std::vector<double> tv(trips.size());
                for (size_t t = 0; t < trips.size(); ++t) { tr[t] = (int32_t)(trips[t].row() - (long)row0); tc[t] = (int32_t)trips[t].col(); tv[t] = trips[t].value(); }
                int b = -1;
                if (!check(admm_hip_add_generic_batch(gpu, (int)(j - i), erp.data(), (int64_t)trips.size(), tr.data(), tc.data(), tv.data(), user_weights.data() + row0, &b))) return false;
                batch_first.push_back((int)i); batch_count.push_back((int)(j - i)); batch_kind.push_back(ADMM_KIND_GENERIC); batch_moving.push_back(false); batch_urow0.push_back((long)row0); batch_body.push_back(nullptr);
                i = j;
                continue;
            }
            if (kind == ADMM_KIND_COLLISION) {           // one force over all nodes -> one element per node
                CollisionForce *cf = static_cast<CollisionForce *>(forces[i].get());
                const int nn_ = dof / 3;
                std::vector<int32_t> idx(nn_); std::vector<double> par(nn_, cf->weight);
                for (int q = 0; q < nn_; ++q) idx[q] = q;
                int b = -1;
                if (!check(admm_hip_add_batch(gpu, kind, nn_, idx.data(), par.data(), nullptr, &b))) return false;
                cf->n_nodes = nn_; cf->Di_rows = dof;
                if (!push_shapes(cf)) return false;
                batch_first.push_back((int)i); batch_count.push_back(1); batch_kind.push_back(kind); batch_moving.push_back(false); batch_urow0.push_back(-1); batch_body.push_back(nullptr);
                ++i;
                continue;
            }
            const bool moving = dynamic_cast<MovingAnchor *>(forces[i].get()) != nullptr;
            // (a run of moving anchors also ends where the body they are fastened to changes; all null: the grouping by kind and flavour alone)
            const CollisionShape *const body = moving ? static_cast<const MovingAnchor *>(forces[i].get())->body.get() : nullptr;
            size_t j = i;
            std::vector<int32_t> idx; std::vector<double> par, tgt;
            const int nn = ADMM_KIND_NODES[kind], np = ADMM_KIND_PARAMS[kind];
            for (; j < forces.size() && forces[j]->kind() == kind && (dynamic_cast<MovingAnchor *>(forces[j].get()) != nullptr) == moving &&
                   (!moving || static_cast<const MovingAnchor *>(forces[j].get())->body.get() == body); ++j) {
                int id[4] = {0, 0, 0, 0}; double p[4] = {0, 0, 0, 0};
                forces[j]->describe(id, p);
                idx.insert(idx.end(), id, id + nn); par.insert(par.end(), p, p + np);
                if (moving) { const MovingAnchor *ma = static_cast<const MovingAnchor *>(forces[j].get()); for (int c = 0; c < 3; ++c) tgt.push_back(ma->point->pos[c]); }
            }
            int b = -1;
            if (!check(admm_hip_add_batch(gpu, kind, (int)(j - i), idx.data(), par.data(), moving ? tgt.data() : nullptr, &b))) return false;
            batch_first.push_back((int)i); batch_count.push_back((int)(j - i)); batch_kind.push_back(kind); batch_moving.push_back(moving); batch_urow0.push_back(-1); batch_body.push_back(body);
            i = j;
        }
        // rigid attachments (MovingAnchor::body; admm_hip_attach_anchors): behind the loop, where every CollisionForce has registered its
        // rigid bodies; the offsets come from the control points and the body's pose as they stand
        for (size_t b = 0; b < batch_body.size(); ++b) if (batch_body[b]) {
            const size_t k = std::find(rigid_shapes.begin(), rigid_shapes.end(), batch_body[b]) - rigid_shapes.begin();
            if (k == rigid_shapes.size()) {
                std::cerr << "\n**Solver Error: force " << batch_first[b] << ": MovingAnchor::body is not a rigid body of a CollisionForce's shape list (rigid_mass > 0, settings.contact_attribution)" << std::endl;
                return false;
            }
            if (!check(admm_hip_attach_anchors(gpu, (int)b, (int)k, nullptr))) return false;
        }
        user_rows = (long)user_weights.size();
        if (user_rows && !check(admm_hip_set_project_hook(gpu, &System::project_hook, this))) return false;
        // ExplicitForce / WindForce run on the device; a user-written subclass stays on the host (step())
        explicit_slot.assign(explicit_forces.size(), -1);
        for (size_t i = 0; i < explicit_forces.size(); ++i) {
            const ExplicitForce &ef = *explicit_forces[i];
            if (!ef.on_device()) continue;
            const double d[3] = {ef.direction[0], ef.direction[1], ef.direction[2]};
            const std::vector<int> &il = ef.index_list();
            const int type = ef.explicit_type();
            const int cnt = (int)il.size() / (type == ADMM_EXPLICIT_WIND ? 3 : 1);
            std::vector<int32_t> il32(il.begin(), il.end());
            if (!check(admm_hip_add_explicit(gpu, type, d, cnt, il32.empty() ? nullptr : il32.data(), &explicit_slot[i]))) return false;
        }
        for (size_t g = 0; g < damping_groups.size(); ++g) {      // (a bad range, an overlap or a bad rate fails here, with the library's message)
            const DampingGroup &d = damping_groups[g];
            if (!check(admm_hip_add_damping_group(gpu, d.node_first, d.node_count < 0 ? dof / 3 - d.node_first : d.node_count, d.drag, d.internal, nullptr))) return false;
        }
        for (size_t c = 0; c < pressure_chambers.size(); ++c) {      // (a bad triangle, an open gas chamber or a bad parameter fails here, with the library's message)
            const PressureChamber &p = pressure_chambers[c];
            if (!check(admm_hip_add_pressure_chamber(gpu, (int)(p.tris.size() / 3), p.tris.data(), p.mode, p.params, nullptr))) return false;
        }
        if (!check(admm_hip_finalize(gpu))) return false;
        // write back what Force::initialize / get_selector compute in the reference
        user_local.clear();
        for (size_t b = 0; b < batch_first.size(); ++b) {
            if (batch_kind[b] == ADMM_KIND_GENERIC) {    // this rank's user forces (all of them on one GPU)
                int nl = 0;
                if (!check(admm_hip_local_elements(gpu, (int)b, nullptr, 0, &nl))) return false;
                std::vector<int32_t> ids(nl > 0 ? nl : 1);
                if (!check(admm_hip_local_elements(gpu, (int)b, ids.data(), nl, &nl))) return false;
                for (int q = 0; q < nl; ++q) user_local.push_back(batch_first[b] + ids[q]);
                continue;
            }
            const int ne = batch_kind[b] == ADMM_KIND_COLLISION ? dof / 3 : batch_count[b];
            std::vector<double> w(ne), rest((size_t)ne * 12); std::vector<int32_t> g(ne);
            if (!check(admm_hip_read_rest(gpu, (int)b, w.data(), rest.data(), g.data()))) return false;
            if (batch_kind[b] == ADMM_KIND_COLLISION) { forces[batch_first[b]]->global_idx = g[0]; continue; }   // weight stays use_weight
            for (int e = 0; e < batch_count[b]; ++e) { Force *f = forces[batch_first[b] + e].get(); f->weight = w[e]; f->global_idx = g[e]; }
        }
        user_Dx.resize(user_rows); user_u.resize(user_rows); user_z.resize(user_rows);
        if (settings.verbose >= 1) std::cout << m_x.size() / 3 << " nodes, " << forces.size() << " forces" << std::endl;
        initialized = true;
        return true;
    }

    // System.cpp:26-75
    bool step() {
        if (!initialized) return false;
        for (size_t cb = 0; cb < pre_step_callbacks.size(); ++cb) pre_step_callbacks[cb](this);
        // host-mutable parameters: control points, explicit-force directions
        for (size_t b = 0; b < batch_first.size(); ++b) if (batch_moving[b]) {
            std::vector<double> &tgt = anchor_tgt; std::vector<int32_t> &act = anchor_act;      // members: no allocation per frame
            tgt.resize((size_t)batch_count[b] * 3); act.resize(batch_count[b]);
            for (int e = 0; e < batch_count[b]; ++e) {
                const MovingAnchor *ma = static_cast<const MovingAnchor *>(forces[batch_first[b] + e].get());
                for (int c = 0; c < 3; ++c) tgt[3 * (size_t)e + c] = ma->point->pos[c];
                act[e] = ma->point->active ? 1 : 0;
            }
            // (an attached batch's control points are the device's: only the flags travel)
            if (!check(admm_hip_update_anchors(gpu, (int)b, batch_body[b] ? nullptr : tgt.data(), act.data()))) return false;
        }
        // user-written explicit forces act on the host copy before it is uploaded (System.cpp:37-39; they run before the
        // device-side ones, in their own relative order)
        for (size_t i = 0; i < explicit_forces.size(); ++i) {
            if (explicit_slot[i] < 0) { explicit_forces[i]->project(settings.timestep_s, m_x, m_v, m_masses); continue; }
            const Vector3d &d = explicit_forces[i]->direction;
            if (!check(admm_hip_set_gravity(gpu, explicit_slot[i], d[0], d[1], d[2]))) return false;
        }
        for (size_t b = 0; b < batch_first.size(); ++b) if (batch_kind[b] == ADMM_KIND_COLLISION && !push_shapes(static_cast<CollisionForce *>(forces[batch_first[b]].get()))) return false;
        // m_x / m_v are public and may have been edited by the caller between steps: they travel every frame, one DMA each
        // way per vector out of / into the vectors' own (page-locked) memory
        pin_state();
        if (!check(admm_hip_upload_state(gpu, m_x.data(), m_v.data()))) return false;
        if (!check(admm_hip_set_tolerance(gpu, settings.residual_tol_primal, settings.residual_tol_dual, settings.residual_check_every < 1 ? 1 : settings.residual_check_every))) return false;
        if (!check(admm_hip_enable_objective(gpu, settings.track_objective ? 1 : 0))) return false;
        if (!check(admm_hip_set_acceleration(gpu, settings.anderson_window))) return false;
        if (!push_reaction_shares(true)) return false;      // (shares that went to zero: before the switch, which cannot go off above them)
        if ((int)settings.contact_attribution != attribution_sent) {      // (on a change only: switching it on clears the record)
            if (!check(admm_hip_enable_contact_attribution(gpu, settings.contact_attribution ? 1 : 0))) return false;
            attribution_sent = (int)settings.contact_attribution;
        }
        if (!push_reaction_shares(false)) return false;     // (shares above zero: behind the switch they need)
        if (!check(admm_hip_step(gpu, settings.admm_iters))) return false;
        if (!check(admm_hip_download_state(gpu, m_x.data(), m_v.data()))) return false;
        // released MovingAnchors follow their node: point->pos = Dx (AnchorForce.cpp:80-83)
        for (size_t b = 0; b < batch_first.size(); ++b) if (batch_moving[b]) {
            bool any_released = false;
            for (int e = 0; e < batch_count[b] && !any_released; ++e) any_released = !static_cast<MovingAnchor *>(forces[batch_first[b] + e].get())->point->active;
            if (!any_released) continue;
            if (shard.world > 1) {
                // sharded: a rank holds the projection state of its own anchors only.  The owner's Dx of the last project() (the
                // reference's value, AnchorForce.cpp:80-83) + zeros elsewhere, summed over the ranks through the iterations' own
                // transport: the control points are the single-GPU run's on every rank
                std::vector<double> &all = anchor_tgt;
                all.assign((size_t)batch_count[b] * 3, 0.0);
                anchor_ids.resize((size_t)batch_count[b]);
                int n_local = 0;
                if (!check(admm_hip_local_elements(gpu, (int)b, anchor_ids.data(), batch_count[b], &n_local))) return false;
                anchor_loc.resize((size_t)(n_local > 0 ? n_local : 1) * 3);
                if (n_local > 0 && !check(admm_hip_read_local(gpu, (int)b, nullptr, nullptr, anchor_loc.data(), nullptr))) return false;
                for (int l = 0; l < n_local; ++l) for (int c = 0; c < 3; ++c) all[3 * (size_t)anchor_ids[l] + c] = anchor_loc[3 * (size_t)l + c];
                if (!check(admm_hip_allreduce_host(gpu, all.data(), (int64_t)all.size()))) return false;
                for (int e = 0; e < batch_count[b]; ++e) {
                    MovingAnchor *ma = static_cast<MovingAnchor *>(forces[batch_first[b] + e].get());
                    if (!ma->point->active) for (int c = 0; c < 3; ++c) ma->point->pos[c] = all[3 * (size_t)e + c];
                }
                continue;
            }
            std::vector<double> &tgt = anchor_tgt;
            tgt.resize((size_t)batch_count[b] * 3);
            if (!check(admm_hip_read_local(gpu, (int)b, nullptr, nullptr, tgt.data(), nullptr))) return false;
            for (int e = 0; e < batch_count[b]; ++e) {
                MovingAnchor *ma = static_cast<MovingAnchor *>(forces[batch_first[b] + e].get());
                if (!ma->point->active) for (int c = 0; c < 3; ++c) ma->point->pos[c] = tgt[3 * (size_t)e + c];
            }
        }
        elapsed_s += settings.timestep_s;
        return true;
    }

    // System.cpp:159-179: Force::weight was edited by the caller
    void recompute_weights() {
        if (!initialized) return;
        // user forces announce their weights through get_selector again (System.cpp:165-168); same call order -> same global_idx
        std::vector<Eigen::Triplet<double> > trips; std::vector<double> user_weights;
        for (size_t i = 0; i < forces.size(); ++i) if (forces[i]->kind() < 0) forces[i]->get_selector(m_x, trips, user_weights);
        if ((long)user_weights.size() != user_rows) { std::cerr << "\n**Solver Error: user forces changed their row count in recompute_weights" << std::endl; return; }
        for (size_t b = 0; b < batch_first.size(); ++b) {
            if (batch_kind[b] == ADMM_KIND_GENERIC) {
                if (!check(admm_hip_set_weights(gpu, (int)b, user_weights.data() + batch_urow0[b]))) return;
                continue;
            }
            const int ne = batch_kind[b] == ADMM_KIND_COLLISION ? (int)m_x.size() / 3 : batch_count[b];
            std::vector<double> w(ne);
            for (int e = 0; e < ne; ++e) w[e] = forces[batch_first[b] + (batch_kind[b] == ADMM_KIND_COLLISION ? 0 : e)]->weight;
            if (!check(admm_hip_set_weights(gpu, (int)b, w.data()))) return;
        }
        check(admm_hip_recompute_weights(gpu));
    }

    // extension, no reference counterpart (admm_hip_energy): the energies of the device state as the last step() left it (m_x / m_v edited
    // since are not uploaded by this call).  ok = false: the call failed (not initialized, no GPU).
    struct Energy { double kinetic, gravity, elastic, anchor; long n_infinite, batches_skipped; bool ok; };
    Energy energy() {
        Energy e = {0.0, 0.0, 0.0, 0.0, 0, 0, false};
        admm_hip_energy_totals t;
        if (!initialized || !check(admm_hip_energy(gpu, &t))) return e;
        e.kinetic = t.kinetic; e.gravity = t.gravity; e.elastic = t.elastic; e.anchor = t.anchor;
        e.n_infinite = (long)t.n_infinite; e.batches_skipped = (long)t.batches_skipped; e.ok = true;
        return e;
    }
    // extension, no reference counterpart (admm_hip_node_forces): the internal forces -sum D_i^T dE_i/dd of the device state as the last
    // step() left it, [n_nodes][3] in m_x's node order; elastic: the built-in elastic forces, anchor: the anchors' (the reaction at a held
    // node is minus its elastic force).  ok = false: the call failed (not initialized, no GPU).
    struct NodeForces { std::vector<double> elastic, anchor; long n_nonfinite, batches_skipped; bool ok; };
    NodeForces node_forces() {
        NodeForces f; f.n_nonfinite = 0; f.batches_skipped = 0; f.ok = false;
        if (!initialized) return f;
        f.elastic.assign((size_t)m_x.size(), 0.0); f.anchor.assign((size_t)m_x.size(), 0.0);
        admm_hip_force_info info;
        if (!check(admm_hip_node_forces(gpu, f.elastic.data(), f.anchor.data(), &info))) { f.elastic.clear(); f.anchor.clear(); return f; }
        f.n_nonfinite = (long)info.n_nonfinite; f.batches_skipped = (long)info.batches_skipped; f.ok = true;
        return f;
    }
    // extension, no reference counterpart (admm_hip_node_reactions): the forces the collision and the anchor constraints exerted on their
    // nodes in the last step(), f = w^2 ((z - u) - x), [n_nodes][3] in m_x's node order; n_contacts: the nodes with depth |u| > 0.
    // ok = false: the call failed (not initialized, no GPU, no step() yet).
    struct NodeReactions { std::vector<double> contact, anchor; long batches_collision, batches_anchor, batches_skipped, n_contacts; bool ok; };
    NodeReactions node_reactions() {
        NodeReactions r; r.batches_collision = r.batches_anchor = r.batches_skipped = r.n_contacts = 0; r.ok = false;
        if (!initialized) return r;
        r.contact.assign((size_t)m_x.size(), 0.0); r.anchor.assign((size_t)m_x.size(), 0.0);
        admm_hip_reaction_info info;
        if (!check(admm_hip_node_reactions(gpu, r.contact.data(), r.anchor.data(), &info))) { r.contact.clear(); r.anchor.clear(); return r; }
        r.batches_collision = (long)info.batches_collision; r.batches_anchor = (long)info.batches_anchor;
        r.batches_skipped = (long)info.batches_skipped; r.n_contacts = (long)info.n_contacts; r.ok = true;
        return r;
    }
    // the nodes in contact (admm_hip_get_contacts): depth > depth_min (a length: above the rounding residue of a free node's u, a few ulp of
    // |x|, below any penetration you care about), ascending node index in m_x's order; empty when none or when the call failed
    std::vector<admm_hip_contact> contacts(double depth_min = 1e-10) {
        std::vector<admm_hip_contact> c;
        if (!initialized) return c;
        c.resize((size_t)m_x.size() / 3);
        int64_t n = 0;
        if (!check(admm_hip_get_contacts(gpu, depth_min, c.data(), (int64_t)c.size(), &n))) n = 0;
        c.resize((size_t)(n < (int64_t)c.size() ? n : (int64_t)c.size()));
        return c;
    }
    // their resultant (admm_hip_contact_resultant): the force and its torque about `pivot`; count < 0: the call failed
    struct ContactResultant { double force[3], torque[3]; long count; };
    ContactResultant contact_resultant(double px = 0.0, double py = 0.0, double pz = 0.0, double depth_min = 1e-10) {
        ContactResultant r = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, -1};
        if (!initialized) return r;
        const double pivot[3] = {px, py, pz};
        double out[6]; int64_t n = 0;
        if (!check(admm_hip_contact_resultant(gpu, depth_min, pivot, out, &n))) return r;
        for (int j = 0; j < 3; ++j) { r.force[j] = out[j]; r.torque[j] = out[3 + j]; }
        r.count = (long)n;
        return r;
    }
    // what the contacts touch, under settings.contact_attribution (admm_hip_get_contact_owners): the nodes of contacts(depth_min) in its
    // order, each with the entry of the shape list that last moved it (-1: none in the last local step), the direction of that push and
    // the node's contact force split into its part along that normal and the rest; empty when none or when the call failed
    std::vector<admm_hip_contact_owner> contact_owners(double depth_min = 1e-10) {
        std::vector<admm_hip_contact_owner> c;
        if (!initialized) return c;
        c.resize((size_t)m_x.size() / 3);
        int64_t n = 0;
        if (!check(admm_hip_get_contact_owners(gpu, depth_min, c.data(), (int64_t)c.size(), &n))) n = 0;
        c.resize((size_t)(n < (int64_t)c.size() ? n : (int64_t)c.size()));
        return c;
    }
    // two-way contact (CollisionBody::reaction_share; admm_hip_get_surface_reaction): what the last step() took off the velocities of the
    // surfaces' nodes, dv [3 n] (0 where nothing landed), one record per contact in contacts()' order, and the counts; ok = false: the
    // call failed
    struct SurfaceReaction { std::vector<double> dv; std::vector<admm_hip_surface_contact> records; admm_hip_surface_reaction_info info; bool ok; };
    SurfaceReaction surface_reaction() {
        SurfaceReaction r;
        r.info = admm_hip_surface_reaction_info(); r.ok = false;
        if (!initialized) return r;
        r.dv.assign((size_t)m_x.size(), 0.0);
        r.records.resize((size_t)m_x.size() / 3);
        int64_t n = 0;
        r.ok = check(admm_hip_get_surface_reaction(gpu, r.dv.data(), r.records.data(), (int64_t)r.records.size(), &n, &r.info));
        if (!r.ok) n = 0;
        r.records.resize((size_t)(n < (int64_t)r.records.size() ? n : (int64_t)r.records.size()));
        return r;
    }
    // rigid bodies (CollisionShape::rigid_mass; admm_hip_get_rigid_state): one record per body in the order of the shape list -- the state
    // c, q, v, L, the derived omega, R and the entry's par, the last frame's applied F, tau and number of contacts.  Empty: none, or the
    // call failed.
    std::vector<admm_hip_rigid_state> rigid_state() {
        std::vector<admm_hip_rigid_state> r(rigid_shapes.size());
        if (!initialized || r.empty() || !check(admm_hip_get_rigid_state(gpu, (int)r.size(), r.data()))) r.clear();
        return r;
    }
    // rigid attachments (MovingAnchor::body; admm_hip_get_attachment): the control points of every attached anchor, as the device moved
    // them at the start of the last step(), into point->pos (a released one: its node's position).  false: the call failed.
    bool attachment_targets() {
        if (!initialized) return false;
        for (size_t b = 0; b < batch_body.size(); ++b) if (batch_body[b]) {
            std::vector<double> &tgt = anchor_tgt;
            tgt.resize((size_t)batch_count[b] * 3);
            if (!check(admm_hip_get_attachment(gpu, (int)b, nullptr, nullptr, tgt.data()))) return false;
            for (int e = 0; e < batch_count[b]; ++e) {
                MovingAnchor *ma = static_cast<MovingAnchor *>(forces[batch_first[b] + e].get());
                for (int c = 0; c < 3; ++c) ma->point->pos[c] = tgt[3 * (size_t)e + c];
            }
        }
        return true;
    }
    // ... and what the bodies carried in the last step() (admm_hip_get_attachment_load): per body, in rigid_state()'s order, the force
    // and the torque about its centre before that step's integration as the nodes felt them (the body received the opposite) and the
    // number of active attached anchors.  Empty: no body, or the call failed.
    struct AttachmentLoad { double force[3], torque[3]; long n_active; };
    std::vector<AttachmentLoad> attachment_load() {
        std::vector<AttachmentLoad> rows;
        const size_t n = rigid_shapes.size();
        if (!initialized || !n) return rows;
        std::vector<double> F(3 * n), T(3 * n); std::vector<int64_t> na(n);
        if (!check(admm_hip_get_attachment_load(gpu, (int)n, F.data(), T.data(), na.data()))) return rows;
        rows.resize(n);
        for (size_t q = 0; q < n; ++q) {
            for (int j = 0; j < 3; ++j) { rows[q].force[j] = F[3 * q + j]; rows[q].torque[j] = T[3 * q + j]; }
            rows[q].n_active = (long)na[q];
        }
        return rows;
    }
    // the contacts' resultant per entry of the shape list (admm_hip_entry_resultants): rows [n_entries + 1], the last one for the contacts
    // that nothing moved in the last local step; n_entries: the length of the CollisionForce's shape list.  Empty: the call failed.
    std::vector<ContactResultant> entry_resultants(int n_entries, double px = 0.0, double py = 0.0, double pz = 0.0, double depth_min = 1e-10) {
        std::vector<ContactResultant> rows;
        if (!initialized || n_entries < 0) return rows;
        const double pivot[3] = {px, py, pz};
        std::vector<double> out(6 * ((size_t)n_entries + 1)); std::vector<int64_t> n((size_t)n_entries + 1);
        if (!check(admm_hip_entry_resultants(gpu, depth_min, pivot, n_entries, out.data(), n.data()))) return rows;
        rows.resize((size_t)n_entries + 1);
        for (size_t q = 0; q < rows.size(); ++q) {
            for (int j = 0; j < 3; ++j) { rows[q].force[j] = out[6 * q + j]; rows[q].torque[j] = out[6 * q + 3 + j]; }
            rows[q].count = (long)n[q];
        }
        return rows;
    }
    // the Cauchy stress of the tets of device batch `batch` (admm_hip_batch_stress): seven doubles per tet, xx, yy, zz, xy, xz, yz, von
    // Mises, in the order of admm_hip_read_local; empty when the call failed (not a tet batch, not initialized, no GPU)
    std::vector<double> batch_stress(int batch) {
        std::vector<double> s;
        int n = 0;
        if (!initialized || !check(admm_hip_local_elements(gpu, batch, nullptr, 0, &n))) return s;
        s.assign((size_t)7 * (n > 0 ? n : 0), 0.0);
        std::vector<double> one(7, 0.0);
        if (!check(admm_hip_batch_stress(gpu, batch, n > 0 ? s.data() : one.data(), nullptr))) s.clear();
        return s;
    }
    // the last step()'s per-iteration histories under settings.track_objective: inertia(x_k), elastic(x_k); their sum is the objective
    struct Objective { std::vector<double> inertia, elastic; };
    Objective objective() {
        Objective o;
        if (!initialized) return o;
        int n = 0;
        if (!check(admm_hip_get_objective(gpu, nullptr, nullptr, 0, &n)) || n <= 0) return o;
        o.inertia.resize(n); o.elastic.resize(n);
        if (!check(admm_hip_get_objective(gpu, o.inertia.data(), o.elastic.data(), n, &n))) { o.inertia.clear(); o.elastic.clear(); }
        return o;
    }

    // the last step()'s Anderson acceleration records under settings.anderson_window > 0, one per ADMM iteration (include/admm_hip.h)
    std::vector<admm_hip_acceleration_record> acceleration_log() {
        std::vector<admm_hip_acceleration_record> log;
        if (!initialized) return log;
        int n = 0;
        if (!check(admm_hip_get_acceleration_log(gpu, nullptr, 0, &n)) || n <= 0) return log;
        log.resize(n);
        if (!check(admm_hip_get_acceleration_log(gpu, log.data(), n, &n))) log.clear();
        return log;
    }

    // extension, no reference counterpart (admm_hip_add_damping_group): velocity damping of the nodes [node_first, node_first + node_count)
    // of m_x's node order (node_count < 0: through the last node), applied on the device after every step(): `drag` (1/s) is ether drag,
    // `internal` (1/s) removes the velocity that is not the group's rigid-body motion, so a flying, spinning body keeps both while its
    // jiggle dies.  Groups are disjoint.  Before initialize() only, which hands them to the library and fails on a bad one; returns the
    // group's id (-1: refused because the system is initialized already).
    struct DampingGroup { int node_first, node_count; double drag, internal; };
    int add_damping_group(int node_first = 0, int node_count = -1, double drag = 0.0, double internal = 0.0) {
        if (initialized) { std::cerr << "\n**Solver Error: add_damping_group after initialize()" << std::endl; return -1; }
        const DampingGroup d = {node_first, node_count, drag, internal};
        damping_groups.push_back(d);
        return (int)damping_groups.size() - 1;
    }
    // new rates of one group (admm_hip_set_damping), in effect from the next step() on; before or after initialize()
    bool set_damping(int group, double drag, double internal) {
        if (group < 0 || group >= (int)damping_groups.size()) { std::cerr << "\n**Solver Error: set_damping: group " << group << " does not exist" << std::endl; return false; }
        if (initialized && !check(admm_hip_set_damping(gpu, group, drag, internal))) return false;
        damping_groups[group].drag = drag; damping_groups[group].internal = internal;
        return true;
    }
    // a group's mass, centre of mass, momentum, angular momentum and inertia about it, angular velocity and kinetic energies from the
    // device state as the last step() left it (admm_hip_get_group_moments); ok = false: the call failed (not initialized, no such group)
    struct GroupMoments { admm_hip_group_moments m; bool ok; };
    GroupMoments group_moments(int group) {
        GroupMoments r; std::memset(&r.m, 0, sizeof r.m); r.ok = false;
        if (!initialized) return r;
        r.ok = check(admm_hip_get_group_moments(gpu, group, &r.m));
        return r;
    }

    // extension, no reference counterpart (admm_hip_add_pressure_chamber): a pressure chamber, oriented triangles tris [nt][3] over m_x's
    // node order with a law -- ADMM_PRESSURE_CONSTANT {p}: the gauge pressure p; ADMM_PRESSURE_GAS {amount, ambient}: p = amount / V -
    // ambient, the chamber must be closed and enclose a positive volume.  Every step() adds dt f / m to the velocities on the device, from
    // the frame-start positions, before gravity and the wind.  Before initialize() only, which hands the chambers to the library and fails
    // on a bad one; returns the chamber's id (-1: refused because the system is initialized already).
    struct PressureChamber { std::vector<int32_t> tris; int mode; double params[2]; };
    int add_pressure_chamber(const std::vector<int> &tris, int mode = ADMM_PRESSURE_CONSTANT, double param0 = 0.0, double param1 = 0.0) {
        if (initialized) { std::cerr << "\n**Solver Error: add_pressure_chamber after initialize()" << std::endl; return -1; }
        PressureChamber p;
        p.tris.assign(tris.begin(), tris.end()); p.mode = mode; p.params[0] = param0; p.params[1] = param1;
        pressure_chambers.push_back(p);
        return (int)pressure_chambers.size() - 1;
    }
    // a new law for one chamber (admm_hip_set_pressure), in effect from the next step() on; before or after initialize()
    bool set_pressure(int chamber, int mode, double param0, double param1 = 0.0) {
        if (chamber < 0 || chamber >= (int)pressure_chambers.size()) { std::cerr << "\n**Solver Error: set_pressure: chamber " << chamber << " does not exist" << std::endl; return false; }
        const double params[2] = {param0, param1};
        if (initialized && !check(admm_hip_set_pressure(gpu, chamber, mode, params))) return false;
        pressure_chambers[chamber].mode = mode; pressure_chambers[chamber].params[0] = param0; pressure_chambers[chamber].params[1] = param1;
        return true;
    }
    // a chamber's volume, area, area vector, pressure and resultant from the device state as the last step() left it
    // (admm_hip_get_chamber_state); ok = false: the call failed (not initialized, no such chamber)
    struct ChamberState { admm_hip_chamber_state s; bool ok; };
    ChamberState chamber_state(int chamber) {
        ChamberState r; std::memset(&r.s, 0, sizeof r.s); r.ok = false;
        if (!initialized) return r;
        r.ok = check(admm_hip_get_chamber_state(gpu, chamber, &r.s));
        return r;
    }

    admm_hip_ctx *context() { return gpu; }

protected:
    bool initialized;
    int attribution_sent = -1;      // settings.contact_attribution as the library last got it (-1: never)
    admm_hip_ctx *gpu;
    std::vector<std::pair<const admm_hip_mesh *, int> > mesh_ids;      // CollisionMesh obstacles registered with the context -> their mesh_id
    std::vector<long> mesh_versions;                                  // ... and the CollisionMesh::version the context last received
    bool friction_pushed = false;                                      // a CollisionShape::friction != 0 went to the context: keep handing the coefficients over
    bool frames_pushed = false;                                        // ... likewise a frame that is not the identity, or a box
    bool motion_pushed = false;                                        // ... likewise a nonzero rigid motion
    std::vector<double> mesh_thick;                                    // the CollisionMesh::half_thickness the context last received
    std::vector<long> mesh_vel_versions;                               // the CollisionMesh::vel_version the context last received
    std::vector<double> body_mu;                                       // the CollisionBody::surface_friction the context last received
    std::vector<std::pair<const CollisionBody *, int> > body_ids;     // CollisionBody surfaces registered with the context -> their mesh_id
    std::vector<const CollisionShape *> rigid_shapes;                  // the shapes registered as rigid bodies, in body order
    std::vector<double> body_share;                                    // the CollisionBody::reaction_share the context last received
    std::vector<int> batch_first, batch_count, batch_kind;
    std::vector<char> batch_moving;
    std::vector<const CollisionShape *> batch_body;      // moving-anchor batches: the rigid body they are fastened to (MovingAnchor::body), else null
    std::vector<long> batch_urow0;         // generic batches: first of their rows among the user rows (-1 otherwise)
    std::vector<int> explicit_slot;        // explicit_forces[i] -> index among the device-side explicit forces, -1 = host
    // user-written forces: their rows of Dx / u / z (the vectors Force::project receives) and this rank's forces
    long user_rows;
    std::vector<int> user_local;
    VectorXd user_Dx, user_u, user_z;
    void *pinned_x, *pinned_v, *seen_x, *seen_v; size_t pinned_bytes;
    std::vector<double> anchor_tgt, anchor_loc; std::vector<int32_t> anchor_act, anchor_ids;     // step(): this frame's control points
    std::vector<DampingGroup> damping_groups;      // add_damping_group's records, handed to the library by initialize()
    std::vector<PressureChamber> pressure_chambers;      // add_pressure_chamber's records, handed to the library by initialize()
    int init_count;                        // initialize() calls so far (every rank counts alike: part of the rendezvous file's name)

    // world > 1: hand rank / world / mode to the library and install the all-reduce -- a caller's hook, or (default) an RCCL
    // communicator inside the library, its id bootstrapped through shard.rccl_id_file
    bool setup_shard() {
        ++init_count;
        if (shard.world <= 1) return true;
        if (shard.rank < 0 || shard.rank >= shard.world) { std::cerr << "\n**Solver Error: shard.rank " << shard.rank << " outside [0, " << shard.world << ")" << std::endl; return false; }
        if (!check(admm_hip_set_shard(gpu, shard.rank, shard.world)) || !check(admm_hip_set_shard_mode(gpu, shard.mode)) || !check(admm_hip_set_factor_local(gpu, shard.factor_local ? 1 : 0))) return false;
        if (shard.host_allreduce) return check(admm_hip_set_host_allreduce(gpu, shard.host_allreduce, shard.host_allreduce_user));
        if (shard.allreduce) return check(admm_hip_set_allreduce(gpu, shard.allreduce, shard.allreduce_user));
        unsigned char id[128];
        std::memset(id, 0, sizeof id);
        if (shard.rank == 0 && !check(admm_hip_rccl_unique_id(id))) return false;
        const std::string file = shard.rccl_id_file.empty() ? std::string() : shard.rccl_id_file + "." + std::to_string(init_count);
        std::string why;
        if (!comm::rccl_id_via_file(file, shard.rank, id, shard.rendezvous_timeout_s, shard.rendezvous_max_age_s, &why)) {
            std::cerr << "\n**Solver Error: multi-GPU rendezvous failed: " << why << " (set System::shard.rccl_id_file / ADMM_HIP_RCCL_ID_FILE to a path unique to this launch, or install an all-reduce hook)" << std::endl;
            return false;
        }
        const bool ok = check(admm_hip_rccl_init(gpu, id, shard.rank, shard.world));     // collective: returns once every rank has joined
        if (shard.rank == 0) std::remove(file.c_str());
        return ok;
    }

    // Force::project for every user force of this rank (System.cpp:57-58), on the rows the library hands over
    static int project_hook(void *self_, double dt, int64_t n_rows, const double *Dx, double *u, double *z) {
        System *self = static_cast<System *>(self_);
        if (n_rows != (int64_t)self->user_rows) return 1;
        const size_t bytes = sizeof(double) * (size_t)n_rows;
        std::memcpy(self->user_Dx.data(), Dx, bytes); std::memcpy(self->user_u.data(), u, bytes); std::memcpy(self->user_z.data(), z, bytes);
        const int nf = (int)self->user_local.size();
        // a team sized to the work (one thread per 512 forces, at most 16): this runs once per ADMM iteration between two GPU
        // phases, and the default team -- every hardware thread of the host, 128+ -- costs milliseconds to wake for microseconds of work
        int team = nf / 512; team = team > 16 ? 16 : (team < 1 ? 1 : team);
#pragma omp parallel for num_threads(team) if (team > 1) schedule(static)
        for (int i = 0; i < nf; ++i) self->forces[self->user_local[i]]->project(dt, self->user_Dx, self->user_u, self->user_z);
        std::memcpy(u, self->user_u.data(), bytes); std::memcpy(z, self->user_z.data(), bytes);
        return 0;
    }

    // page-lock m_x / m_v where they lie (again if the caller resized them)
    void pin_state() {
        const size_t bytes = sizeof(double) * (size_t)m_x.size();
        if (seen_x == (void *)m_x.data() && seen_v == (void *)m_v.data() && pinned_bytes == bytes) return;
        unpin_state();
        seen_x = m_x.data(); seen_v = m_v.data(); pinned_bytes = bytes;       // tried once per buffer: pageable memory still works, just slower
        if (admm_hip_pin_host(gpu, m_x.data(), bytes, 1) == ADMM_OK) pinned_x = m_x.data();
        if (admm_hip_pin_host(gpu, m_v.data(), bytes, 1) == ADMM_OK) pinned_v = m_v.data();
    }
    void unpin_state() {
        if (gpu && pinned_x) admm_hip_pin_host(gpu, pinned_x, pinned_bytes, 0);
        if (gpu && pinned_v) admm_hip_pin_host(gpu, pinned_v, pinned_bytes, 0);
        pinned_x = pinned_v = seen_x = seen_v = nullptr; pinned_bytes = 0;
    }
    void release() {
        unpin_state();
        if (gpu) { admm_hip_destroy(gpu); gpu = nullptr; }
        mesh_ids.clear(); mesh_versions.clear(); body_ids.clear(); friction_pushed = false;
        motion_pushed = false; frames_pushed = false; mesh_vel_versions.clear(); mesh_thick.clear(); body_mu.clear(); body_share.clear(); rigid_shapes.clear();
        initialized = false; attribution_sent = -1;
    }

    bool push_shapes(const CollisionForce *cf) {
        std::vector<int32_t> ty; std::vector<double> par;
        for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
            const CollisionShape &sh = *cf->collisionShapes[q];
            ty.push_back(sh.shape_type());
            par.push_back(sh.center[0]); par.push_back(sh.center[1]); par.push_back(sh.center[2]);
            if (sh.shape_type() == ADMM_SHAPE_MESH && (typeid(sh) == typeid(CollisionBody) || typeid(sh) == typeid(CollisionSheet))) {      // a body surface (a sheet: an open one): registered once, then it follows its nodes
                const CollisionBody &cb = static_cast<const CollisionBody &>(sh);
                size_t k = 0;
                while (k < body_ids.size() && body_ids[k].first != &cb) ++k;
                if (k == body_ids.size()) {
                    int id = -1;
                    const std::vector<int32_t> t(cb.tris.begin(), cb.tris.end());
                    const CollisionSheet *cs = dynamic_cast<const CollisionSheet *>(&cb);
                    if (!check(cs ? admm_hip_add_sheet_surface(gpu, cb.node_first, cb.node_count, (int)(t.size() / 3), t.data(), cs->half_thickness, &id)
                                  : admm_hip_add_body_surface(gpu, cb.node_first, cb.node_count, (int)(t.size() / 3), t.data(), &id))) return false;
                    if (cs && cs->self_collision && !check(admm_hip_set_sheet_self_collision(gpu, id, 1))) return false;
                    if (!cs && cb.self_collision[0] != 0.0 && !check(admm_hip_set_body_self_collision(gpu, id, cb.self_collision[0], cb.self_collision[1], cb.self_collision[2]))) return false;
                    if (cs && cs->side_reach != 0.0 && !check(admm_hip_set_collision_mesh_side_memory(gpu, id, cs->side_reach))) return false;
                    body_ids.push_back(std::make_pair(&cb, id));
                    body_mu.push_back(0.0);
                }
                if (body_mu[k] != cb.surface_friction) {
                    if (!check(admm_hip_set_body_surface_friction(gpu, body_ids[k].second, cb.surface_friction))) return false;
                    body_mu[k] = cb.surface_friction;
                }
                par.push_back((double)body_ids[k].second);
            } else if (sh.shape_type() == ADMM_SHAPE_MESH) {      // a mesh: registered with the context once (before finalize), then named by its id
                const CollisionMesh &cm = static_cast<const CollisionMesh &>(sh);
                const admm_hip_mesh *m = cm.mesh.get();
                size_t k = 0;
                while (k < mesh_ids.size() && mesh_ids[k].first != m) ++k;
                if (k == mesh_ids.size()) {
                    int id = -1;
                    if (!check(admm_hip_add_collision_mesh(gpu, m, &id))) return false;
                    if (cm.side_reach != 0.0 && !check(admm_hip_set_collision_mesh_side_memory(gpu, id, cm.side_reach))) return false;
                    mesh_ids.push_back(std::make_pair(m, id));
                    mesh_versions.push_back(cm.version);
                    mesh_vel_versions.push_back(0);
                    mesh_thick.push_back(cm.half_thickness);
                } else if (mesh_versions[k] != cm.version) {      // deformed since the context last saw it (CollisionMesh::set_vertices)
                    if (!check(admm_hip_update_collision_mesh(gpu, mesh_ids[k].second, (int)(cm.vertices.size() / 3), cm.vertices.data()))) return false;
                    mesh_versions[k] = cm.version;
                }
                if (mesh_thick[k] != cm.half_thickness) {      // an open mesh's half thickness, changed since the context last saw it
                    if (!check(admm_hip_set_collision_mesh_thickness(gpu, mesh_ids[k].second, cm.half_thickness))) return false;
                    mesh_thick[k] = cm.half_thickness;
                }
                // its vertex velocities, once the context is finalized (the library takes them from then on: step() calls this every frame)
                if (initialized && mesh_vel_versions[k] != cm.vel_version) {
                    if (!check(admm_hip_set_collision_mesh_velocity(gpu, mesh_ids[k].second, (int)(cm.velocities.size() / 3), cm.velocities.empty() ? nullptr : cm.velocities.data()))) return false;
                    mesh_vel_versions[k] = cm.vel_version;
                }
                par.push_back((double)mesh_ids[k].second);
            } else if (sh.shape_type() == ADMM_SHAPE_BOX) {       // a box: its half extents; its centre goes into the frame below
                const CollisionBox &bx = static_cast<const CollisionBox &>(sh);
                for (int j = 0; j < 3; ++j) par[par.size() - 3 + j] = bx.half[j];
                par.push_back(0.0);
            } else {
                par.push_back(sh.shape_radius());
            }
        }
        if (!check(admm_hip_set_collision_shapes(gpu, (int)ty.size(), ty.data(), par.data()))) return false;
        // the shapes' frames (contexts that never saw a turned shape or a box skip the call: every frame is the identity anyway)
        std::vector<double> fr(12 * cf->collisionShapes.size());
        bool oriented = false;
        for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
            const CollisionShape &sh = *cf->collisionShapes[q];
            sh.frame(sh.frame_pivot(), &fr[12 * q]);
            oriented = oriented || sh.shape_type() == ADMM_SHAPE_BOX;
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) oriented = oriented || sh.orientation[i][j] != (i == j ? 1.0 : 0.0);
        }
        if (oriented || frames_pushed) {
            frames_pushed = true;
            if (!check(admm_hip_set_collision_frames(gpu, (int)cf->collisionShapes.size(), fr.data()))) return false;
        }
        // rigid bodies (CollisionShape::rigid_mass > 0; admm_hip_add_rigid_body): registered once, behind the frames; they need the
        // attribution switch, which otherwise travels with the first step()
        for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
            const CollisionShape &sh = *cf->collisionShapes[q];
            if (!(sh.rigid_mass > 0.0) || std::find(rigid_shapes.begin(), rigid_shapes.end(), &sh) != rigid_shapes.end()) continue;
            if (settings.contact_attribution && attribution_sent != 1) {
                if (!check(admm_hip_enable_contact_attribution(gpu, 1))) return false;
                attribution_sent = 1;
            }
            const Vector3d c = sh.rigid_com_set ? sh.rigid_com : (sh.shape_type() == ADMM_SHAPE_SPHERE ? sh.center : sh.frame_pivot());
            const double com[3] = {c[0], c[1], c[2]}, acc[3] = {sh.rigid_accel[0], sh.rigid_accel[1], sh.rigid_accel[2]};
            if (!check(admm_hip_add_rigid_body(gpu, (int)q, sh.rigid_mass, sh.rigid_inertia, com, acc, nullptr))) return false;
            rigid_shapes.push_back(&sh);
        }
        // the shapes' friction coefficients (contexts that never saw one above 0 skip the call: they run the frictionless kernels anyway)
        std::vector<double> mu;
        bool any = false;
        for (size_t q = 0; q < cf->collisionShapes.size(); ++q) { mu.push_back(cf->collisionShapes[q]->friction); any = any || mu.back() != 0.0; }
        if (any || friction_pushed) {
            friction_pushed = true;
            if (!check(admm_hip_set_collision_friction(gpu, (int)mu.size(), mu.data()))) return false;
        }
        // ... and their rigid motions, the same way
        std::vector<double> mo;
        bool moving = false;
        for (size_t q = 0; q < cf->collisionShapes.size(); ++q) {
            const CollisionShape &sh = *cf->collisionShapes[q];
            for (int j = 0; j < 3; ++j) mo.push_back(sh.lin_velocity[j]);
            for (int j = 0; j < 3; ++j) mo.push_back(sh.ang_velocity[j]);
            for (int j = 0; j < 3; ++j) mo.push_back(sh.pivot[j]);
        }
        for (size_t i = 0; i < mo.size(); ++i) moving = moving || mo[i] != 0.0;
        if (!moving && !motion_pushed) return true;
        motion_pushed = true;
        return check(admm_hip_set_collision_motion(gpu, (int)cf->collisionShapes.size(), mo.data()));
    }

    // CollisionBody::reaction_share of every registered surface, on a change only (admm_hip_set_surface_reaction); zeros: the shares that
    // are now zero, else the others
    bool push_reaction_shares(bool zeros) {
        body_share.resize(body_ids.size(), 0.0);
        for (size_t k = 0; k < body_ids.size(); ++k) {
            const double s = body_ids[k].first->reaction_share;
            if (s == body_share[k] || (s == 0.0) != zeros) continue;
            if (!check(admm_hip_set_surface_reaction(gpu, body_ids[k].second, s))) return false;
            body_share[k] = s;
        }
        return true;
    }

    bool check(int rc) {
        if (rc == ADMM_OK) return true;
        std::cerr << "\n**Solver Error (admm_hip " << rc << "): " << (gpu ? admm_hip_last_error(gpu) : "no context") << std::endl;
        return false;
    }
};

} // namespace admm
