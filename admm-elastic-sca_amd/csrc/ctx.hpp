// ctx.hpp -- the library's context (admm_hip_ctx) and the host-side records it is made of, shared by the library's translation units:
//   admm_hip.hip     device code (kernels_*.hpp, factor_dev.hpp) + device factorization, upload, launches, step loop, C ABI
//   host_setup.cpp   Force::initialize / get_selector data, assembly of A_s, ordering + symbolic / host numeric factorization
//   partition.cpp    subtree sharding: owners of supernodes and elements
//   comm.cpp         RCCL (bound at run time) and the all-reduce hooks + their C ABI entry points
// See include/admm_hip.h for the contract and DESIGN.md for the design.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/admm_hip.h"
#include "factor.hpp"
#include "dev_types.hpp"
#include "mesh_host.hpp"
#include "node_csr.hpp"
#include "collision_plan.hpp"
#include "sweep_plan.hpp"
#include "rigid.hpp"

namespace admm_lib {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Batch {
    int kind = 0, n_total = 0, n_local = 0;
    std::vector<int32_t> local;    // this rank's elements (ascending reference order); contiguous range unless subtree sharding
    std::vector<int32_t> idx;      // [n_total][nodes] original ids
    std::vector<double> params;    // [n_total][P]
    std::vector<double> targets;   // anchors [n_total][3]
    bool moving = false;
    std::vector<int32_t> active;   // anchors [n_total]
    double *h_tg = nullptr; int32_t *h_ac = nullptr; hipEvent_t upd_ev = nullptr;   // anchors: pinned staging of this rank's targets / flags + "last update has left it"
    // finalize
    std::vector<double> weight, rest, measure;  // [n_total], [n_total][12], [n_total]
    std::vector<int32_t> global_idx;             // compact first row
    std::vector<int32_t> corner_perm;            // [n_total][nodes]: stored corner c holds original corner corner_perm[c]
    int64_t slot_base = 0;                       // first local force slot
    int max_iter = 0;                            // largest L-BFGS max_iterations (hyperelastic kinds)
    // device
    int *d_idx = nullptr, *d_dst = nullptr, *d_active = nullptr, *d_niters = nullptr;
    int *d_order = nullptr; unsigned int *d_cost = nullptr; int n_blocks_ordered = 0;      // tets: launch order by last frame's cost (see project_tet_kernel)
    double *d_rest = nullptr, *d_par = nullptr, *d_w2h2 = nullptr, *d_kblend = nullptr, *d_w2 = nullptr;
    double *d_u = nullptr, *d_z = nullptr, *d_state = nullptr, *d_targets = nullptr;
    double *d_dx_override = nullptr, *d_dx_buf = nullptr; // parity tests only
    double *d_u_prev = nullptr, *d_z_prev = nullptr, *d_G = nullptr;   // residual tracking only
    // tets: the corners' right-hand-side shares are summed per node inside every 64-tet block (LDS) before they go to the slots:
    // one slot per (block, node) instead of one per corner (project_tet_kernel's epilogue)
    bool prered = false;
    int tpb = 64;      // tets per one-wave block (admm_hip_ctx::tet_tpb): 64, or fewer in under-filled launches -- the lanes beyond stay idle
    unsigned int *d_pos4 = nullptr; int *d_bn_ptr = nullptr, *d_bn_dst = nullptr; unsigned short *d_bn_end = nullptr;
    double *d_res_partial = nullptr; bool res_fused = false;           // tets: residuals come out of the projection kernel itself (one |r|^2 partial per 64-tet block)
    // energies (kernels_energy.hpp): the elements' scale s, uploaded at finalize; the per-element values, one partial and one count of
    // non-finite elements per 64-element block, allocated by the first call that evaluates an energy (abi_energy.inc)
    double *d_escale = nullptr, *d_eE = nullptr, *d_epart = nullptr; int *d_ecnt = nullptr;
    // gradients (kernels_gradient.hpp), allocated by the first call that evaluates one (abi_gradient.inc): g SoA [rows][n_local], one count
    // of non-finite elements per 64-element block, the batch's corner forces at gr_cf_off of the context's d_gr_cf; tets, first
    // admm_hip_batch_stress: the stress SoA [7][n_local] and the rest volumes
    double *d_gg = nullptr, *d_gstress = nullptr, *d_gvol = nullptr; int *d_gcnt = nullptr; long long gr_cf_off = 0;
    std::vector<double> G;                // [12][n_local] selector block per element, corners in device order
    long long rx_off = 0;                 // reactions (abi_reaction.inc): where a collision / anchor batch's rows sit in the context's d_rx_el
    long long at_off = 0;                 // contact attribution (abi_reaction.inc): where a collision batch's elements sit in the context's d_at_owner / d_at_normal
    long long aa_off_z = 0, aa_off_u = 0; // Anderson acceleration (abi_anderson.inc): where the batch's z and u sit in every state-sized buffer
    // rigid attachments (abi_attach.inc; anchors only): the body the whole batch is fastened to (-1: none), its elements' offsets in the
    // body's own coordinates [n_total][3], and the device's copy of this rank's [n_local][3] (allocated by the first attachment, kept)
    int attach_body = -1; std::vector<double> attach_local; double *d_attach_local = nullptr;
    // ---- ADMM_KIND_GENERIC (user-defined forces): selector rows as CSR over the batch's rows
    std::vector<int64_t> g_elem_row;      // [n_total + 1] first batch row of every element
    std::vector<int64_t> g_rowptr;        // [rows + 1]
    std::vector<int32_t> g_col;           // entry columns (3 * node + component, original node ids), ascending inside a row
    std::vector<double> g_val, g_roww;    // entry values; weight per row
    std::vector<int64_t> g_elem_node;     // [n_total + 1]
    std::vector<int32_t> g_nodes;         // every element's nodes, ascending
    int64_t g_row0 = 0, g_rows = 0;       // position in the context-wide generic row space
    int g_lrows = 0, g_lslots = 0;        // this rank's rows / (element, node) slots
    std::vector<double> g_sval; std::vector<int32_t> g_srow_b;   // per slot entry: D value and batch row (coefficients are rebuilt on recompute_weights)
    int *d_g_lrow = nullptr, *d_g_rptr = nullptr, *d_g_col = nullptr, *d_g_sptr = nullptr, *d_g_srow = nullptr, *d_g_sdst = nullptr;
    double *d_g_val = nullptr, *d_g_scoef = nullptr, *d_g_scoef_res = nullptr;   // (_res: val * w^2, the dual residual's coefficients)
    int elem_nodes(int e, const int32_t **p) const {
        if (kind == ADMM_KIND_GENERIC) { *p = g_nodes.data() + g_elem_node[e]; return (int)(g_elem_node[e + 1] - g_elem_node[e]); }
        *p = idx.data() + (size_t)e * ADMM_KIND_NODES[kind]; return ADMM_KIND_NODES[kind];
    }
    int elem_rows(int e) const { return kind == ADMM_KIND_GENERIC ? (int)(g_elem_row[e + 1] - g_elem_row[e]) : ADMM_KIND_ROWS[kind]; }
};

struct Explicit {
    int type = 0; double dir[3] = {0, 0, 0};
    std::vector<int32_t> idx;            // CONST: node ids (empty = all); WIND: [n][3] triangle node ids
    int n = 0;                            // nodes / triangles
    int *d_idx = nullptr;                 // WIND: triangles sorted by dependency level (see wind_serial_kernel)
    int *d_level_ptr = nullptr; int n_levels = 0;
};

// one level of one pass of the sweeps on the device: the item lists and choices of its LevelPlan (sweep_plan.hpp), uploaded
struct LevelDev {
    int n_small = 0; admm_dev::SweepItem *d_small = nullptr;   // forward: wave items (levels of supernodes with k <= fwd_small_k)
    int n_big = 0, big_nw = 16; admm_dev::SweepItem *d_big = nullptr;   // forward: block items; waves per tile (4 / 8 / 16 by the level's widest supernode)
    using Root = SweepRoot;
    std::vector<Root> roots;                                   // roots solved with their explicit inverse: gather + one row-wise product (no backward items)
    int n_bwd = 0, bwd_cw = 1, bwd_nw = 4; admm_dev::SweepItem *d_bwd = nullptr;   // backward: columns per wave, waves per block
    int level = 0; double mbytes = 0.0;                        // diagnostics: position in the tree, panel bytes of this level's supernodes
};

} // namespace admm_lib

using admm_lib::Batch; using admm_lib::Explicit; using admm_lib::LevelDev;
using admm_host::SymCSC; using admm_host::Factor;

struct admm_hip_ctx {
    int device_id = -1;
    bool own_stream = false;
    hipStream_t stream = nullptr;
    std::string err;
    double dt = 0.04;
    int rank = 0, world = 1;
    admm_hip_allreduce_fn allreduce = nullptr; void *allreduce_user = nullptr;
    void *rccl_comm = nullptr; bool rccl_owned = false;      // ncclComm_t: the all-reduce is ncclAllReduce on the context's stream (takes precedence over the hook)
    admm_hip_host_allreduce_fn host_allreduce = nullptr; void *host_allreduce_user = nullptr;   // transport that sums HOST buffers (admm_hip_set_host_allreduce)
    double *h_comm = nullptr; size_t h_comm_cap = 0;          // its pinned staging
    double *d_small = nullptr; size_t d_small_cap = 0;        // admm_hip_allreduce_host's device scratch
    bool finalized = false;
    // a recompute_weights that failed (not positive definite, HIP error) leaves no usable factor: step / solve_only / local_step_* refuse
    // with ADMM_ERR_STATE and factor_error until a later recompute_weights succeeds (require_factor)
    bool factor_invalid = false; std::string factor_error;
    int leaf_size = 0;                        // nested-dissection leaf size; 0 = by system size (host_factor)
    // host state
    int n_nodes = 0;
    std::vector<double> x, v, m3;
    std::vector<Batch> batches;
    admm_dev::Gravity grav{};             // fast path: only constant all-node forces
    std::vector<Explicit> explicits; bool explicit_simple = true;
    admm_dev::ShapeTable shapes{}; admm_dev::ShapeTable *d_shapes = nullptr;
    // triangle meshes named by ADMM_SHAPE_MESH entries, registered before finalize (admm_hip_add_collision_mesh: an obstacle;
    // admm_hip_add_body_surface / admm_hip_add_sheet_surface: a surface of simulated nodes): with at least one, the collision batches run
    // project_collision_mesh_kernel instead of a segment of project_multi_kernel.  One record per mesh, indexed by mesh id (mesh_by_id):
    // everything the host knows about it; its arrays are uploaded at finalize, the device tables parallel to d_meshes are built from the
    // records (collision_plan.hpp: plan_mesh_tables; upload.inc)
    // admm_hip_update_collision_mesh after finalize (kernels_mesh.hpp) rewrites a mesh's device arrays in place; the host copy then
    // keeps only the topology.  Every buffer the update needs is allocated at finalize, one set per mesh:
    struct MeshUpdate {
        admm_mesh::Node *nodes; admm_mesh::Tri *tris; admm_mesh::Nrm *nrm;       // the live arrays (d_meshes points at them)
        double *verts, *fn, *vn, *part;                                          // staged vertices, face / vertex normals, volume partials
        int *cid, *adj, *inc_ptr, *inc, *lvl_nodes;                              // the topology (admm_hip_mesh)
        // body surfaces only (else null): the device node id of every vertex, the surface's own check and its BodyStatus
        int *dnode; admm_mesh::UpdateCheck *chk; admm_mesh::BodyStatus *status;
    };
    struct CollisionMesh {
        admm_hip_mesh mesh;
        // what the mesh is to the scene: its owner, the node range [own_first, own_first + own_count) whose collision elements skip it
        // (own_count 0: none; admm_hip_set_collision_mesh_owner), and for a body surface the node behind every vertex, ascending -- the
        // device rebuilds it from them at every step (launch.inc: update_bodies)
        // self_collision (a sheet surface only, admm_hip_set_sheet_self_collision): its own nodes meet it outside their 1-ring instead of skipping it
        // side_reach (an open mesh only, admm_hip_set_collision_mesh_side_memory): > 0: the mesh has side memory with this reach, 0: none
        // body_self (a closed body surface only, admm_hip_set_body_self_collision): {r, R, rho}, r > 0: its surface nodes meet it outside what
        // is near them in the rest shape; rest: the vertices [nv][3] as admm_hip_add_body_surface registered them
        int own_first = 0, own_count = 0; std::vector<int> body_nodes; bool self_collision = false; double side_reach = 0.0;
        double body_self[3] = {0.0, 0.0, 0.0}; std::vector<double> rest;
        // how it moves (admm_hip_set_collision_mesh_velocity, admm_hip_set_body_surface_friction; an entry's rigid motion is
        // shapes.motion).  d_vel: an obstacle's vertex velocities, allocated by the call that first sets them (has_vel: in effect); a
        // body surface's are allocated at finalize and gathered from the frame-start v at every step (launch.inc: update_bodies).
        // body_mu: a body surface's coefficient.
        double *d_vel = nullptr; bool has_vel = false; double body_mu = 0.0; std::vector<double> vel;
        MeshUpdate upd{};             // the device buffers (finalize; all null in a host-only context)
        // two-way contact (admm_hip_set_surface_reaction; a surface of simulated nodes only): the share of a contact's reaction its
        // triangle's corners receive, 0: none; share_dirty: the device's table entry is older
        double reaction_share = 0.0; bool share_dirty = false;
        int side_row = -1;            // its row of d_side / h_side (finalize; -1: no side memory)
        bool body() const { return !body_nodes.empty(); }         // a surface of simulated nodes, not an obstacle
        bool open() const { return mesh.thickness > 0.0; }        // a thick shell, not a closed mesh
    };
    std::vector<CollisionMesh> meshes; admm_mesh::MeshDev *d_meshes = nullptr; admm_mesh::UpdateCheck *d_mesh_chk = nullptr;
    admm_mesh::MeshMotion *d_mesh_motion = nullptr;      // per mesh, parallel to d_meshes: what the moving friction kernel reads (upload.inc: mesh_motion_table)
    // open meshes (thick shells, admm_hip_mesh::thickness > 0): the half thickness of every mesh, parallel to d_meshes (0: a closed mesh), a
    // table of its own that project_collision_shell_kernel alone reads; admm_hip_set_collision_mesh_thickness writes one entry
    double *d_mesh_thick = nullptr;
    // contexts where some sheet collides with itself (else null): the flag of every mesh, parallel to d_meshes; contexts where a sheet or a
    // body surface collides with itself (else null): for every node in device order its vertex id on the self-colliding surface that owns
    // it (-1: none); the self, sided and bodyself collision kernels read them
    int *d_mesh_self = nullptr, *d_self_vid = nullptr;
    // contexts where some open mesh has side memory (mesh_query.hpp; else all null / empty): per mesh, parallel to d_meshes, its reach (0:
    // none), its row in d_side (-1: none) and its boundary table (null: none); d_side [n_side_slots][n_nodes] in device node order, one
    // int32 side per node and mesh with memory.  collision_side_kernel writes d_side at the start of every step,
    // project_collision_sided_kernel reads all four.  CollisionMesh::side_row: the host's copy of the rows; h_side: the sides of a
    // host-only context (caller's node order).
    double *d_mesh_reach = nullptr; int *d_mesh_side_slot = nullptr; const int **d_mesh_bnd = nullptr; int32_t *d_side = nullptr;
    int n_side_slots = 0; std::vector<int32_t> h_side;
    // contexts where some body surface collides with itself (mesh_query.hpp; else both null): per mesh, parallel to d_meshes, the three
    // lengths {r, R, rho} (zeros: off) and the rest vertices [nv][3] (null: none); project_collision_bodyself_kernel alone reads them, with
    // d_self_vid for the nodes' vertex ids
    double *d_mesh_bself = nullptr; const double **d_mesh_rest = nullptr;
    int *d_body_tag = nullptr;      // contexts with an owner: the owner group of every node in device order (-1: none), for MeshDev::owner
    SymCSC A;
    Factor F;
    admm_hip_info info{};
    // device state (node arrays in factor order)
    double *d_x = nullptr, *d_v = nullptr, *d_m3 = nullptr, *d_mxbar = nullptr, *d_xcur = nullptr, *d_y = nullptr, *d_w = nullptr, *d_c = nullptr;
    double *d_fslot = nullptr; int64_t n_fslots = 0;
    int *d_perm = nullptr; double *d_stage = nullptr;          // frame boundary: factor position -> caller's node; [2][3n] staging in the caller's order
    int slot_stride = 0;                      // > 0: RHS slots rank-major (slot of a node's r-th incidence = r * slot_stride + node), 0: node-sorted
    int64_t *d_inc_ptr = nullptr;
    double *d_panels = nullptr; int *d_sn_first = nullptr, *d_sn_ncols = nullptr, *d_sn_nrows = nullptr, *d_rows = nullptr, *d_cg_slot = nullptr, *d_cg4 = nullptr;
    int64_t *d_sn_panel_off = nullptr, *d_sn_rows_off = nullptr, *d_sn_slot_off = nullptr, *d_sn_front_off = nullptr, *d_cg_ptr = nullptr;
    std::vector<LevelDev> levels;
    std::vector<void *> allocs;
    // subtree sharding (world > 1, ADMM_HIP_SHARD=subtree / admm_hip_set_shard_mode): every rank owns whole subtrees of the
    // elimination tree and the elements that touch them; only the top of the tree is replicated
    int shard_mode = 0;                       // 0: contiguous element ranges + replicated solve, 1: subtrees
    std::vector<int> sn_owner, node_owner;    // -1 = top (replicated); node_owner in factor order
    std::vector<LevelDev> levels_top;         // sweep items of the top supernodes (levels = this rank's own ones)
    // rank-local factorization (admm_hip_set_factor_local): under subtree sharding a rank assembles, factors and keeps only its own subtrees and
    // the replicated top; the subtree roots' update matrices meet in ONE all-reduce per factorization (dev_factorize.inc).  The device's panel
    // layout is then a compact one over those supernodes (dev_panel_off; -1 = not resident) -- Factor::panel_off stays the host layout.
    bool factor_local = true, factor_local_on = false;      // wanted / in effect (set by plan_device_panels at finalize)
    std::vector<int64_t> dev_panel_off, dev_root_inv_off; int64_t dev_panels_size = 0;
    // distributed top (host_setup.cpp host_factor): the top of the tree is ONE root supernode, its product with the explicit inverse split by rows across the ranks
    // ADMM_HIP_DIST_TOP = 0: the replicated top of rounds 2-5, 1: distributed whatever the size; default (-1): distributed from dist_top_min_nodes nodes on -- its
    // second collective per iteration costs more than it saves on small systems (1M-tet bar, 178.6k nodes, 8 ranks: the slowest rank's kernels 0.264 -> 0.253 ms for one
    // more all-reduce; 4M tets, 693k nodes: 1.113 -> 0.689 ms)
    int dist_top_wanted = -1, dist_top_min_nodes = 300000; bool dist_top = false;
    int root_sn = -1, root_k = 0, root_first = 0, root_r0 = 0, root_r1 = 0; int64_t root_foff = 0;      // the root, this rank's rows [r0, r1) of its inverse (at dev_root_inv_off[root_sn])
    bool tet_order = true; int tet_order_min_blocks = 3072;      // NH / StVK batches of more blocks than that start their costliest blocks first (ADMM_HIP_TET_ORDER=0: mesh order)
    int64_t frames = 0;
    int merge_small = 0;                          // dissection regions of at most that many nodes become four-way tree nodes (ADMM_HIP_MERGE_SMALL)
    bool fuse_anchor_tail = true;                 // an anchor batch right behind a tet batch goes out in the tet launch (ADMM_HIP_FUSE_ANCHORS=0: own launch)
    bool device_factor = true, device_numeric = false;      // numeric factorization on the GPU (ADMM_HIP_FACTOR=host: on the host); what this context does
    // the tet kernels' z is an output nobody reads back in a plain frame (admm_hip_read_local aside): admm_hip_keep_z(ctx, 0) -- what
    // the class mirror and the bench do -- stops storing it in admm_hip_step; the parity entry points (local_step_only / local_step_dx)
    // and residual tracking always store it.  ADMM_HIP_KEEP_Z=0 / 1 overrides.
    bool keep_z = true, keep_z_user = true;
    bool state_zero_copy = true;              // upload_state / download_state address the caller's page-locked vectors from ONE kernel each (any size; ADMM_HIP_STATE_ZEROCOPY=0: a DMA per vector + reordering kernels)
    int tet_tpb = 0;                          // ADMM_HIP_TPB: tets per one-wave block (4 / 8 / 16 / 32 / 64) for the NH / StVK batches; 0 = 64
    bool tet_prered = true;                   // ADMM_HIP_PRERED=0: one RHS slot per tet corner (the round-1/2 layout)
    int n_comm_top = 0, n_comm_slots = 0;
    int *d_comm_top = nullptr, *d_comm_slots = nullptr; unsigned char *d_comm_mine = nullptr, *d_base_mask = nullptr, *d_keep_mask = nullptr;
    double *d_comm_buf = nullptr;
    // small systems: explicit inverse of the scalar system (factor order), one kernel per solve
    int dense_max = 2048; bool dense = false; std::vector<double> Ainv; double *d_ainv = nullptr;
    // one ADMM iteration (local kernels, RHS, all sweep launches) captured as a HIP graph: one launch per iteration
    // instead of 30-40; matters for the small shipped scenes, which are launch-bound.  Not used around timed iterations, with
    // residual tracking or user forces, or under sharding with a host hook (ncclAllReduce inside the library is capturable:
    // ADMM_HIP_GRAPH_COMM=1).  ADMM_HIP_GRAPH=0 disables.
    // Default (graph_forced = false): only for systems of < 100k nodes, where an iteration is ~20 short dependent kernels and the
    // host's launch work matters; at 1M tets the GPU is the limit and a replay is 0.5-2 % SLOWER than the same launches issued
    // eagerly (0.780 vs 0.766-0.775 ms per iteration, tools/graph_vs_eager.py).  ADMM_HIP_GRAPH=1 forces it, 0 disables it.
    bool graph_enabled = true, graph_forced = false; hipGraph_t iter_graph = nullptr; hipGraphExec_t iter_exec = nullptr;
    // the whole ADMM loop of a frame as ONE graph (one launch per frame instead of one per iteration: the ~5-9 us between two graph
    // launches are 5-15 % of an iteration on small and mid-size scenes); captured for the iteration count of the call, again when it changes
    bool frame_graph_on = true; hipGraph_t frame_graph = nullptr; hipGraphExec_t frame_exec = nullptr; int frame_iters = 0, last_step_iters = -1;
    bool local_multi = true;                      // the whole local step in ONE launch when the scene has several batches (project_multi_kernel; ADMM_HIP_LOCAL_MULTI=0: one launch per batch)
    // class API frame boundary of small systems: no DMA, the permutation kernels read / write this page-locked buffer ([x | v], caller's order)
    int state_direct_max_nodes = 12288; double *h_state = nullptr, *h_state_dev = nullptr; size_t h_state_cap = 0; int *d_iperm = nullptr; hipEvent_t state_in_ev = nullptr; bool state_in_pending = false;
    std::vector<std::pair<const char *, size_t> > pinned;      // host spans page-locked through admm_hip_pin_host (the zero-copy state kernels check them)
    std::vector<double> bounce;                                 // upload_state / download_state of a vector that is page-locked only in part (neither mappable nor DMA-able as one span)
    bool tree_search = true;                       // pick the elimination tree of mid-size systems by the sweeps' cost model (ADMM_HIP_TREE_SEARCH=0: the rule-based tree)
    bool top_bwd_needed_only = true;              // subtree sharding: the backward sweep over the replicated top skips the separators this rank never reads (ADMM_HIP_TOP_BWD_ALL=1: all of them)
    int root_fuse_k = 2048;                       // roots of at most that many columns: t is gathered inside the product kernel (ADMM_HIP_ROOT_FUSE_K; 0 = never)
    admm_lib::SweepKnobs knobs;                   // what the plan of the sweeps reads (sweep_plan.hpp): kernel shapes per level, the fused bottom subtrees
    // the fused launches over the bottom subtrees, one workgroup per subtree (sweep_plan.hpp plan_fused_subtrees):
    int fuse_cut = -1, n_fuse = 0, fuse_lds = 0;  // cut level (-1: nothing fused), subtrees, dynamic LDS bytes of the fused launches
    int *d_fuse_rec = nullptr; int64_t *d_fuse_off = nullptr;      // the subtrees' records (ints) and their offsets [n_fuse + 1]
    // ... and the backward sweep's, over those of them whose backward record fits the LDS cap as well (bwd_record.hpp)
    int n_fuse_bwd = 0, fuse_bwd_lds = 0;
    int *d_fuse_bwd_rec = nullptr; int64_t *d_fuse_bwd_off = nullptr;
    int64_t graph_launches = 0;               // hipGraphLaunch calls so far (admm_hip_debug_graph_state)
    bool graphs_stale = false;                // a captured iteration holds the communicator it was captured with: set when that changes (comm.cpp), honoured by the next admm_hip_step
    bool graph_comm = false;                  // ADMM_HIP_GRAPH_COMM=1: also capture the multi-GPU iteration (ncclAllReduce inside the graph)
    // residual tracking / early exit (off by default)
    bool res_on = false, res_ready = false;
    double tol_r = 0.0, tol_s = 0.0; int check_every = 1;
    double *d_res = nullptr; int res_cap = 0, res_n = 0;      // [2 * res_cap]: r^2, s^2 per iteration
    double *d_res_slots = nullptr, *d_res_s = nullptr, *d_res_partial = nullptr; int res_partial_n = 0;
    // energies and the per-iteration objective (abi_energy.inc; off by default, every buffer created on first use).  d_en_out: { kinetic,
    // gravity, inertia, one total per batch }, d_en_cnt: one count of non-finite elements per batch; d_en_npart: the node terms' partials
    // (kinetic / inertia first, then the constant explicit forces' in list order).  d_obj [obj_cap][1 + batches]: per ADMM iteration of
    // the last step, inertia(x_k) and every batch's total at x_k
    bool en_ready = false; double *d_en_out = nullptr, *d_en_npart = nullptr; long long *d_en_cnt = nullptr;
    bool obj_on = false; int obj_cap = 0, obj_n = 0; double *d_obj = nullptr;
    // gradients and nodal forces (abi_gradient.inc; every buffer created on first use).  d_gr_cf: every evaluated batch's corner forces,
    // SoA [3 nodes][n_local] per batch; d_gr_out [2][3 n_nodes]: the elastic and the anchor forces in the caller's node order; the two
    // CSRs of gradient_gather_kernel (0: elastic batches, 1: anchor batches), built by the first admm_hip_node_forces
    bool gr_ready = false, gr_csr_ready = false; double *d_gr_cf = nullptr, *d_gr_out = nullptr; admm_lib::NodeCsr gr_csr[2];
    // reactions of the collision and anchor batches (abi_reaction.inc; every buffer created by the first call).  d_rx_el: every reported
    // batch's elements, SoA [7][n_local] per batch at Batch::rx_off (f, depth, z); d_rx_node: f_contact [n][3], f_anchor [n][3], depth [n],
    // point [n][3] in the caller's node order; the two CSRs of reaction_gather_kernel (0: collision batches, 1: anchor batches); d_rx_blk:
    // the compaction's block counts, then their offsets; d_rx_count: the contacts' count; d_rx_rec [n_nodes] records; d_rx_part: the
    // resultant's partials [6][n_part] (one row of the per-entry sums; abi_reaction.inc entry_work), then its six totals
    bool rx_ready = false; double *d_rx_el = nullptr, *d_rx_node = nullptr, *d_rx_part = nullptr; int *d_rx_blk = nullptr; long long *d_rx_count = nullptr; void *d_rx_rec = nullptr; admm_lib::NodeCsr rx_csr[2];
    // contact attribution (admm_hip_enable_contact_attribution; abi_reaction.inc, attribution.hpp; off by default).  attribution: the
    // switch, which makes every collision batch launch form 8 (collision_plan.hpp).  The record, allocated by the switch once finalized or
    // by finalize, never by admm_hip_step: at_total elements over the collision batches (a batch's slice at Batch::at_off), d_at_owner
    // [at_total] the last mover of every element (-1: none), d_at_normal SoA [3][at_total] its normal.  The reports' buffers, created by the
    // first report: d_at_rec [n_nodes] owner records, d_at_blk the per-entry block counts, then their offsets, d_at_tot the entries'
    // counts, d_at_perm the contacts sorted by entry, d_at_part the per-entry partials [6][n_part], d_at_out the rows (carved by abi_reaction.inc entry_work)
    bool attribution = false, at_ready = false; long long at_total = 0; int *d_at_owner = nullptr; double *d_at_normal = nullptr;
    void *d_at_rec = nullptr; int *d_at_blk = nullptr, *d_at_perm = nullptr; long long *d_at_tot = nullptr, *d_at_csr = nullptr; double *d_at_part = nullptr, *d_at_out = nullptr;
    // velocity damping per node group (abi_damping.inc, kernels_damping.hpp, damping.hpp; no group = off, the default).  damp_groups: the
    // caller's groups in the order they were added; rate_dirty: the device's rate entry is older than drag / internal.  Device side, created
    // by upload_all when there is a group: the block -> (group, first node) table, the groups' ranges, their rates (written by
    // damping_set_rate_kernel from kernel arguments, at the start of the first filter that runs after a change), the moments records,
    // v_c [groups][3] and the stages' partials [9][damp_blocks]
    struct DampGroupHost { int node_first = 0, node_count = 0; double drag = 0.0, internal = 0.0; bool rate_dirty = true; };
    std::vector<DampGroupHost> damp_groups;
    int damp_blocks = 0; void *d_damp_blk = nullptr, *d_damp_grp = nullptr, *d_damp_rate = nullptr, *d_damp_mom = nullptr; double *d_damp_vc = nullptr, *d_damp_part = nullptr;
    // pressure chambers (abi_pressure.inc, kernels_pressure.hpp, pressure.hpp; no chamber = off, the default).  chambers: the caller's
    // chambers in the order they were added, tris in the caller's node ids; law_dirty: the device's law entry is older than mode / par.
    // Device side, created by upload_all when there is a chamber: the block -> (chamber, first triangle) table, the chambers' ranges,
    // their laws (written by pressure_set_law_kernel from kernel arguments, at the start of the first frame that runs after a change),
    // the records, the collapse counters, the triangles' corners as device positions, their chamber, their normals [3][pres_tris], the
    // partials [5][pres_blocks] and the node CSR of the gather over the pres_nodes distinct chamber nodes
    struct PressureChamberHost { std::vector<int32_t> tris; int mode = 0; double par[2] = {0.0, 0.0}; bool law_dirty = true; };
    std::vector<PressureChamberHost> chambers;
    int pres_blocks = 0, pres_tris = 0, pres_nodes = 0;
    void *d_pres_blk = nullptr, *d_pres_chm = nullptr, *d_pres_law = nullptr, *d_pres_rec = nullptr; long long *d_pres_collapsed = nullptr, *d_pres_off = nullptr;
    int *d_pres_tri = nullptr, *d_pres_trichm = nullptr, *d_pres_node = nullptr, *d_pres_ptr = nullptr, *d_pres_stride = nullptr; double *d_pres_nrm = nullptr, *d_pres_part = nullptr;
    // two-way contact (abi_surface_reaction.inc, kernels_surface_reaction.hpp, surface_reaction.hpp; every share 0 = off, the default).
    // sr_depth_min: the depth above which a node counts as in contact (admm_hip_set_surface_reaction_depth); sr_frame: the value of
    // `frames` after the last step that ran the reaction (-1: none).  Device side, allocated by the first share set in a finalized
    // context or by finalize, never by admm_hip_step: sr_cap contacts at most (the nodes that carry a collision element), sr_nb blocks of
    // 64 shares, sr_passes sort passes; d_sr_mesh the per-mesh table (vertex -> caller's node, share), d_sr_rec [sr_cap] records,
    // d_sr_key / d_sr_idx [2][3 sr_cap] the keys and the shares' indices (ping-pong), d_sr_val [3 sr_cap][3] the contributions, d_sr_blk
    // the sort's block counts, then their offsets ([256][sr_nb] each), d_sr_tot its 256 totals, d_sr_n [6] the shares of the last reacting
    // frame and, behind them, the report's five counts, d_sr_dv [n_nodes][3] in the caller's node order
    double sr_depth_min = 0.0; long long sr_frame = -1; bool sr_ready = false; int sr_cap = 0, sr_nb = 0, sr_passes = 1;
    void *d_sr_mesh = nullptr, *d_sr_rec = nullptr; int *d_sr_key = nullptr, *d_sr_idx = nullptr, *d_sr_blk = nullptr, *d_sr_tot = nullptr;
    double *d_sr_val = nullptr, *d_sr_dv = nullptr; long long *d_sr_n = nullptr;
    // rigid bodies in the collision list (abi_rigid.inc, kernels_rigid.hpp, rigid.hpp; no body = off, the default).  rigid: the bodies in
    // the order they were added -- their constants, the inertia as given, the host's copy of the record (as registered, as last set or
    // as admm_hip_get_rigid_state last read it) and accel_dirty: the device's constants hold an older accel.  rg_depth_min: the depth
    // above which a node's contact loads a body.  Device side, allocated by finalize or by the first admm_hip_add_rigid_body of a
    // finalized context, never by admm_hip_step: d_rg_table the RigidTable (row -> body, the constants), d_rg_rec [ADMM_MAX_SHAPES] the
    // records, d_rg_out [ADMM_MAX_SHAPES][6] the bodies' rows of the entry sums
    struct RigidBodyHost { admm_rigid::Const K; double inertia[6]; admm_rigid::Record rec; bool accel_dirty = false; };
    std::vector<RigidBodyHost> rigid;
    double rg_depth_min = 0.0; bool rg_ready = false;
    void *d_rg_table = nullptr, *d_rg_rec = nullptr; double *d_rg_out = nullptr;
    // rigid attachments (abi_attach.inc, kernels_attach.hpp, attach.hpp; no attached batch = off, the default; a batch's own record is
    // Batch::attach_body / attach_local).  Device side, allocated by finalize or by the first admm_hip_attach_anchors of a finalized
    // context, never by admm_hip_step, for every anchor batch the context has: d_att_bat the attached batches' descriptors, d_att_blk the
    // targets' block -> (batch, first element) table, d_att_slot / d_att_elem the attached elements sorted by (body, batch, element),
    // d_att_total / d_att_carry [ADMM_MAX_SHAPES] the elements per body and whether it carries a batch, d_att_part [6][att_pcap] and
    // d_att_cnt [att_pcap] the load's block partials and active counts, d_att_out [ADMM_MAX_SHAPES][6] the bodies' attachment rows,
    // d_att_nact their active elements.  att_slots / att_tblk / att_pblk: attached batches, blocks of the targets and of the load now.
    bool att_ready = false; int att_slots = 0, att_tblk = 0, att_pblk = 0, att_pcap = 0;
    void *d_att_bat = nullptr, *d_att_blk = nullptr; int *d_att_slot = nullptr, *d_att_elem = nullptr, *d_att_carry = nullptr, *d_att_cnt = nullptr;
    long long *d_att_total = nullptr, *d_att_nact = nullptr; double *d_att_part = nullptr, *d_att_out = nullptr;
    // Anderson acceleration (abi_anderson.inc, kernels_anderson.hpp; window 0 = off, the default; every buffer created by the first step
    // that needs it, again when the window grows).  aa_T: doubles per state-sized vector (all batches' z and u, each segment at an even
    // offset), aa_nblk: blocks of the elementwise launches; d_aa_ring, allocated for the window aa_cap_m, used as [2][aa_m + 1][aa_T]: the history's g, then its f;
    // d_aa_log [aa_log_cap]: one record per iteration of the last step
    int aa_m = 0, aa_cap_m = 0, aa_nblk = 0, aa_log_cap = 0, aa_log_n = 0; long long aa_T = 0; bool aa_ran = false;
    void *d_aa_seg = nullptr, *d_aa_state = nullptr; admm_hip_acceleration_record *d_aa_log = nullptr;
    double *d_aa_sin = nullptr, *d_aa_ring = nullptr, *d_aa_part = nullptr;

    // user-defined forces: host round trip per ADMM iteration (see admm_hip_add_generic_batch)
    admm_hip_project_fn project_hook = nullptr; void *project_user = nullptr;
    int64_t n_gen_rows = 0;
    double *d_gen_dx = nullptr, *d_gen_q = nullptr;                 // [n_gen_rows]
    double *h_gen_dx = nullptr, *h_gen_u = nullptr, *h_gen_z = nullptr, *h_gen_q = nullptr;   // pinned
    std::vector<double> h_gen_u_prev, h_gen_z_prev; double *d_gen_q2 = nullptr, *d_gen_r2 = nullptr;   // residual tracking of the user rows
    hipEvent_t gen_ev = nullptr;
    // timing: HIP events around the phases of every timing_stride-th ADMM iteration (1 = every iteration); an event is a
    // barrier packet that costs ~5 us of launch overlap, so the other iterations run event-free (as a graph replay when one exists)
    bool timing = false; int timing_stride = 1; int ev_timed = 0; int timing_frame = 0;
    std::vector<hipEvent_t> evpool;   // recorded in order during a step, read back lazily
    size_t ev_used = 0; int ev_iters = 0; bool ev_pending = false;
    // the step BEFORE the last one keeps its events (the two sets swap at the start of every timed step): a caller that reads them
    // through admm_hip_get_timing_previous after queueing the next step never makes the GPU wait for the host (bench.py)
    std::vector<hipEvent_t> evpool_prev; size_t ev_used_prev = 0; int ev_iters_prev = 0, ev_timed_prev = 0; bool ev_pending_prev = false;
    admm_hip_timing last_timing{};
};

namespace admm_lib {

int fail(admm_hip_ctx *c, int code, const char *fmt, ...);      // (comm.cpp)

// (a failed call also leaves HIP's sticky last-error set: cleared here, so that an unrelated hipGetLastError() check later -- in this context or
//  another one of the process -- does not report this failure a second time as its own)
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (void)hipGetLastError(); return fail(ctx, ADMM_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } } while (0)

// the record of a registered mesh; null, with the refusal every entry point gives an unknown id, where there is none
inline admm_hip_ctx::CollisionMesh *mesh_by_id(admm_hip_ctx *ctx, int mesh_id) {
    if (mesh_id >= 0 && mesh_id < (int)ctx->meshes.size()) return &ctx->meshes[mesh_id];
    fail(ctx, ADMM_ERR_ARG, "mesh_id %d is not a registered mesh (have %d)", mesh_id, (int)ctx->meshes.size());
    return nullptr;
}
// the record that entry j of a shape list (types [n], params [n][4]) names; null: not a mesh entry, or no such mesh
inline const admm_hip_ctx::CollisionMesh *entry_mesh(const admm_hip_ctx *ctx, const int32_t *types, const double *params, int j) {
    if (types[j] != ADMM_SHAPE_MESH) return nullptr;
    const int id = (int)params[4 * (size_t)j + 3];
    return id >= 0 && id < (int)ctx->meshes.size() ? &ctx->meshes[id] : nullptr;
}

template <class T> int dalloc(admm_hip_ctx *ctx, T **p, size_t n) {
    *p = nullptr;
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    ctx->allocs.push_back(q);
    *p = (T *)q;
    return ADMM_OK;
}
template <class T> int upload(admm_hip_ctx *ctx, T **p, const std::vector<T> &h) {
    int rc = dalloc(ctx, p, h.size());
    if (rc) return rc;
    if (!h.empty()) HIPCHK(hipMemcpy(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return ADMM_OK;
}
#define TRY(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

// is local element `el` the last one of its launch block?
inline bool block_end(const Batch &b, int el) { return el % b.tpb == b.tpb - 1; }
// number of launch blocks of a batch (tets: `tpb` elements per block; everything else LOCAL_BLOCK)
inline int batch_blocks(const Batch &b) { return (b.n_local + b.tpb - 1) / b.tpb; }

// ---- what one translation unit offers the others ----
int do_allreduce(admm_hip_ctx *ctx, double *buf, int64_t count);                                   // comm.cpp
void comm_release(admm_hip_ctx *ctx);
int comm_poll(admm_hip_ctx *ctx, int *nccl_result);
int host_assemble(admm_hip_ctx *ctx, bool reuse_rest);                                             // host_setup.cpp
int host_factor(admm_hip_ctx *ctx, bool reuse_symbolic);
void element_G(int kind, const double *rest, double G[4][3], int &cols);
int idx_stride(int kind);
void partition_subtrees(admm_hip_ctx *ctx);                                                        // partition.cpp
void assign_elements(admm_hip_ctx *ctx);
int check_split_elements(admm_hip_ctx *ctx);
void top_needs(const admm_hip_ctx *ctx, std::vector<std::vector<char> > &need, std::vector<int> &provider);
void shard_accounting(admm_hip_ctx *ctx);
void plan_device_panels(admm_hip_ctx *ctx);
void subtree_owners(const admm_host::Factor &F, int parts, std::vector<int> &owner, std::vector<double> &load, int &n_top, size_t &n_sub);

} // namespace admm_lib
