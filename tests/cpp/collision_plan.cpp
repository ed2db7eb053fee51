// collision_plan.hpp against what it must equal.  collision_form_of: a hand-written table of shape lists and mesh facts with the form,
// own_launch and sided each must give.  plan_mesh_tables: every output against brute force written here, for each node and mesh directly
// from the definition.  Stand-alone: includes collision_plan.hpp alone, exits 0 when every case agrees.
#include "collision_plan.hpp"

#include <cstdio>
#include <vector>

using namespace admm_lib;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// ---- the form ------------------------------------------------------------------------------------------------------------------------
// one entry of a list: its type, the mesh id of a mesh entry, its coefficient, whether it has a rigid motion / a frame that is not the identity
struct Entry { int type; int mesh; double mu; bool moves, framed; };
static const Entry FLOOR{ADMM_SHAPE_FLOOR, -1, 0.0, false, false}, SPHERE{ADMM_SHAPE_SPHERE, -1, 0.0, false, false}, BOX{ADMM_SHAPE_BOX, -1, 0.0, false, false};
static Entry mesh_entry(int id, double mu = 0.0) { return Entry{ADMM_SHAPE_MESH, id, mu, false, false}; }
static Entry with_mu(Entry e, double mu) { e.mu = mu; return e; }
static Entry moving(Entry e) { e.moves = true; return e; }
static Entry framed(Entry e) { e.framed = true; return e; }

// the first n of `entries` are the list; what follows sits in the table behind it and must be ignored
static admm_dev::ShapeTable table_of(const std::vector<Entry> &entries, int n) {
    admm_dev::ShapeTable S{};
    S.n = n;
    for (size_t j = 0; j < entries.size(); ++j) {
        const Entry &e = entries[j];
        S.type[j] = e.type;
        S.par[j][0] = S.par[j][1] = S.par[j][2] = e.type == ADMM_SHAPE_BOX ? 0.5 : 0.0;
        S.par[j][3] = e.type == ADMM_SHAPE_MESH ? (double)e.mesh : 1.0;
        S.mu[j] = e.mu;
        if (e.moves) S.motion[j][4] = 0.25;      // one component of the angular velocity
        for (int k = 0; k < 12; ++k) S.frame[j][k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        S.framed[j] = e.framed ? 1 : 0;
    }
    return S;
}

// facts with one trait each (what the library's setters allow together does not bind the pure function)
static const MeshFacts PLAIN{false, 0.0, false, 0.0, 0.0, 0.0, false};                 // a closed obstacle
static const MeshFacts WITH_VEL{false, 0.0, false, 0.0, 0.0, 0.0, true};               // ... with vertex velocities
static const MeshFacts BODY{true, 0.0, false, 0.0, 0.0, 0.0, false};                   // a closed body surface
static const MeshFacts BODY_MU{true, 0.0, false, 0.0, 0.0, 0.4, false};                // ... with a coefficient
static const MeshFacts OBSTACLE_MU{false, 0.0, false, 0.0, 0.0, 0.4, false};           // a stray body_mu on an obstacle counts for nothing
static const MeshFacts SHELL{false, 0.02, false, 0.0, 0.0, 0.0, false};                // an open mesh
static const MeshFacts SELF{true, 0.0, true, 0.0, 0.0, 0.0, false};                    // self_collision alone
static const MeshFacts SIDED{false, 0.0, false, 0.1, 0.0, 0.0, false};                 // a reach alone
static const MeshFacts BODYSELF{true, 0.0, false, 0.0, 0.01, 0.0, false};              // a half gap alone
static const MeshFacts ALL{true, 0.02, true, 0.1, 0.01, 0.4, true};                    // every trait

static void check_form(const char *name, const std::vector<Entry> &entries, const std::vector<MeshFacts> &meshes, int form, bool own_launch, bool sided, int n = -1) {
    const admm_dev::ShapeTable S = table_of(entries, n < 0 ? (int)entries.size() : n);
    int asked = 0;
    const CollisionForm f = collision_form_of(S, (int)meshes.size(), [&](int id) { ++asked; return meshes[(size_t)id]; });
    if (f.form != form || f.own_launch != own_launch || f.sided != sided)
        std::printf("  %s: form %d own_launch %d sided %d, expected %d %d %d\n", name, f.form, (int)f.own_launch, (int)f.sided, form, (int)own_launch, (int)sided);
    CHECK(f.form == form && f.own_launch == own_launch && f.sided == sided);
    CHECK(asked <= S.n);      // one pass: a mesh's facts are asked for once per entry that names it at the most
}

static void form_cases() {
    std::printf("the form of a list\n");
    check_form("the empty list", {}, {}, 0, false, false);
    check_form("the empty list, a mesh registered", {}, {ALL}, 0, true, false);
    check_form("analytic shapes only", {FLOOR, SPHERE}, {}, 0, false, false);
    check_form("analytic shapes only, a mesh with every trait registered but unnamed", {FLOOR, SPHERE}, {ALL}, 0, true, false);
    check_form("a trait-free mesh named, one with every trait unnamed", {FLOOR, mesh_entry(0)}, {PLAIN, ALL}, 0, true, false);
    // each trigger alone
    check_form("1 alone: a coefficient", {FLOOR, with_mu(SPHERE, 0.3)}, {}, 1, true, false);
    check_form("2 alone: a coefficient and a motion", {moving(with_mu(SPHERE, 0.3))}, {}, 2, true, false);
    check_form("2 alone: a coefficient on a mesh with velocities", {mesh_entry(0, 0.3)}, {WITH_VEL}, 2, true, false);
    check_form("2 alone: a body surface with a coefficient", {mesh_entry(0)}, {BODY_MU}, 2, true, false);
    check_form("3 alone: a framed entry", {framed(SPHERE)}, {}, 3, true, false);
    check_form("3 alone: a box", {BOX}, {}, 3, true, false);
    check_form("4 alone: an open mesh", {mesh_entry(0)}, {SHELL}, 4, true, false);
    check_form("5 alone: a sheet that collides with itself", {mesh_entry(0)}, {SELF}, 5, true, false);
    check_form("6 alone: a mesh with side memory", {mesh_entry(0)}, {SIDED}, 6, true, true);
    check_form("7 alone: a body that collides with itself", {mesh_entry(0)}, {BODYSELF}, 7, true, false);
    // each trigger with the one below it, in either order of the entries
    check_form("1 with 0", {SPHERE, with_mu(FLOOR, 0.2)}, {}, 1, true, false);
    check_form("2 with 1", {with_mu(FLOOR, 0.2), moving(with_mu(SPHERE, 0.3))}, {}, 2, true, false);
    check_form("3 with 2", {framed(SPHERE), moving(with_mu(SPHERE, 0.3))}, {}, 3, true, false);
    check_form("4 with 3", {BOX, mesh_entry(0)}, {SHELL}, 4, true, false);
    check_form("5 with 4", {mesh_entry(1), mesh_entry(0)}, {SHELL, SELF}, 5, true, false);
    check_form("6 with 5", {mesh_entry(0), mesh_entry(1)}, {SIDED, SELF}, 6, true, true);
    check_form("7 with 6", {mesh_entry(1), mesh_entry(0)}, {SIDED, BODYSELF}, 7, true, true);
    check_form("every trigger at once", {BOX, moving(with_mu(FLOOR, 0.2)), mesh_entry(0)}, {ALL}, 7, true, true);
    // the edge cases
    check_form("7 beside a mesh with memory that no entry names: no latch", {mesh_entry(1)}, {SIDED, BODYSELF}, 7, true, false);
    check_form("a motion without a coefficient", {moving(SPHERE)}, {}, 0, false, false);
    check_form("a motion without a coefficient beside a coefficient without a motion", {moving(SPHERE), with_mu(FLOOR, 0.2)}, {}, 1, true, false);
    check_form("a mesh with velocities named without a coefficient", {mesh_entry(0)}, {WITH_VEL}, 0, true, false);
    check_form("a mesh with velocities named without a coefficient, another entry with one", {mesh_entry(0), with_mu(FLOOR, 0.2)}, {WITH_VEL}, 1, true, false);
    check_form("a body surface with a coefficient, the entry's own 0", {FLOOR, mesh_entry(1, 0.0)}, {BODY, BODY_MU}, 2, true, false);
    check_form("a body surface without a coefficient", {mesh_entry(0)}, {BODY, BODY_MU}, 0, true, false);
    check_form("an obstacle's body_mu counts for nothing", {mesh_entry(0)}, {OBSTACLE_MU}, 0, true, false);
    check_form("a box without any frame, no mesh", {FLOOR, BOX}, {}, 3, true, false);
    check_form("a mesh id past the registered ones", {mesh_entry(2), mesh_entry(-1)}, {ALL, ALL}, 0, true, false);
    // entry n, just past the list's length, holds every trigger and is ignored
    check_form("every trigger in entry n", {FLOOR, framed(moving(mesh_entry(0, 0.3)))}, {ALL}, 0, true, false, 1);
    check_form("a box in entry n", {SPHERE, BOX}, {}, 0, false, false, 1);
    check_form("every trigger in entry 0 of an empty list", {framed(moving(mesh_entry(0, 0.3)))}, {ALL}, 0, true, false, 0);
    // the same trait-free mesh twice
    check_form("a trait-free mesh named twice", {mesh_entry(0), FLOOR, mesh_entry(0)}, {PLAIN}, 0, true, false);
    check_form("a full table", std::vector<Entry>(ADMM_MAX_SHAPES, mesh_entry(0)), {SHELL}, 4, true, false);
}

// ---- the tables ----------------------------------------------------------------------------------------------------------------------
struct MeshCase { int own_first, own_count; std::vector<int> body_nodes; bool self_collision; double body_self[3]; double side_reach; };

static bool same_range(const MeshCase &a, const MeshCase &b) { return a.own_first == b.own_first && a.own_count == b.own_count; }
// the owner group of mesh i by the definition: groups are numbered in the order their range first appears among the meshes
static int brute_owner(const std::vector<MeshCase> &M, size_t i) {
    if (!M[i].own_count) return -1;
    size_t first = i;
    for (size_t j = i; j-- > 0;) if (M[j].own_count && same_range(M[j], M[i])) first = j;
    int g = 0;
    for (size_t j = 0; j < first; ++j) {
        if (!M[j].own_count) continue;
        bool seen = false;
        for (size_t k = 0; k < j; ++k) seen |= M[k].own_count && same_range(M[k], M[j]);
        g += seen ? 0 : 1;
    }
    return g;
}

static void check_tables(const char *name, int n_nodes, const std::vector<int> &iperm, const std::vector<MeshCase> &M) {
    std::printf("%s\n", name);
    const int failures_before = failures;
    std::vector<MeshPlanInput> in;
    for (const MeshCase &m : M)
        in.push_back(MeshPlanInput{m.own_first, m.own_count, m.body_nodes.data(), (int)m.body_nodes.size(), m.self_collision, {m.body_self[0], m.body_self[1], m.body_self[2]}, m.side_reach});
    const MeshTables T = plan_mesh_tables(n_nodes, iperm.data(), in);
    const size_t nm = M.size();
    bool any_owner = false, any_sheet = false, any_body = false; int n_rows = 0;
    for (const MeshCase &m : M) {
        any_owner |= m.own_count != 0; any_sheet |= m.self_collision; any_body |= !m.self_collision && m.body_self[0] > 0.0; n_rows += m.side_reach > 0.0 ? 1 : 0;
    }
    // which tables exist: the ones whose device pointer the upload sets
    CHECK(T.owner.size() == nm && T.side_row.size() == nm);
    CHECK(T.any_sheet_self == any_sheet && T.any_body_self == any_body && T.n_side_rows == n_rows);
    CHECK(T.tag.size() == (any_owner ? (size_t)n_nodes : 0));
    CHECK(T.self_flag.size() == (any_sheet ? nm : 0));
    CHECK(T.vid.size() == (any_sheet || any_body ? (size_t)n_nodes : 0));
    CHECK(T.body_self.size() == (any_body ? 3 * nm : 0));
    if (failures != failures_before) return;      // (the sizes are off: nothing to index)
    for (size_t i = 0; i < nm; ++i) {
        CHECK(T.owner[i] == brute_owner(M, i));
        int row = -1;
        if (M[i].side_reach > 0.0) { row = 0; for (size_t j = 0; j < i; ++j) row += M[j].side_reach > 0.0 ? 1 : 0; }
        CHECK(T.side_row[i] == row);
        if (any_sheet) CHECK(T.self_flag[i] == (M[i].self_collision ? 1 : 0));
        if (any_body) for (int j = 0; j < 3; ++j) CHECK(T.body_self[3 * i + j] == (M[i].body_self[0] > 0.0 ? M[i].body_self[j] : 0.0));
    }
    for (int p = 0; p < n_nodes; ++p) {      // device position p holds the caller's node k
        int k = -1;
        for (int q = 0; q < n_nodes; ++q) if (iperm[q] == p) k = q;
        CHECK(k >= 0);
        int tag = -1, vid = -1;
        for (size_t i = 0; i < nm; ++i) {
            if (M[i].own_count && k >= M[i].own_first && k < M[i].own_first + M[i].own_count) tag = brute_owner(M, i);
            if (M[i].self_collision || M[i].body_self[0] > 0.0)
                for (size_t v = 0; v < M[i].body_nodes.size(); ++v) if (M[i].body_nodes[v] == k) vid = (int)v;
        }
        if (any_owner) CHECK(T.tag[p] == tag);
        if (any_sheet || any_body) CHECK(T.vid[p] == vid);
    }
}

static void table_cases() {
    const std::vector<int> iperm7{3, 0, 6, 1, 5, 2, 4}, id7{0, 1, 2, 3, 4, 5, 6};
    const MeshCase sheet_self{0, 4, {0, 1, 3}, true, {0.0, 0.0, 0.0}, 0.0};                // a sheet on nodes [0, 4) that collides with itself
    const MeshCase shares{0, 4, {}, false, {0.0, 0.0, 0.0}, 0.1};                          // an obstacle owned by the same range, with side memory
    const MeshCase body_self{4, 3, {4, 5, 6}, false, {0.01, 0.02, 0.03}, 0.0};             // a body on nodes [4, 7) that collides with itself
    const MeshCase no_owner{0, 0, {}, false, {0.0, 0.0, 0.0}, 0.2};                        // an obstacle without an owner, with side memory
    const MeshCase plain_body{4, 3, {6, 4}, false, {0.0, 0.0, 0.0}, 0.0};                  // a body surface that does not collide with itself
    const MeshCase plain{0, 0, {}, false, {0.0, 0.0, 0.0}, 0.0};
    check_tables("7 nodes, four meshes: two share a range, one disjoint, one without an owner", 7, iperm7, {sheet_self, shares, body_self, no_owner});
    check_tables("... the disjoint range first, the unowned mesh between", 7, iperm7, {body_self, no_owner, shares, sheet_self});
    check_tables("... with the identity permutation", 7, id7, {sheet_self, shares, body_self, no_owner});
    {
        const std::vector<MeshCase> M{sheet_self, shares, body_self, no_owner};
        std::vector<MeshPlanInput> in;
        for (const MeshCase &m : M) in.push_back(MeshPlanInput{m.own_first, m.own_count, m.body_nodes.data(), (int)m.body_nodes.size(), m.self_collision, {m.body_self[0], m.body_self[1], m.body_self[2]}, m.side_reach});
        const MeshTables T = plan_mesh_tables(7, iperm7.data(), in);      // ... and by hand
        CHECK((T.owner == std::vector<int>{0, 0, 1, -1}) && (T.side_row == std::vector<int>{-1, 0, -1, 1}) && T.n_side_rows == 2);
        CHECK((T.tag == std::vector<int>{0, 0, 1, 0, 1, 1, 0}));       // device positions 0..6 hold nodes 1, 3, 5, 0, 6, 4, 2
        CHECK((T.vid == std::vector<int>{1, 2, 1, 0, 2, 0, -1}));
        CHECK((T.self_flag == std::vector<int>{1, 0, 0, 0}) && T.body_self[6] == 0.01 && T.body_self[8] == 0.03 && T.body_self[0] == 0.0);
    }
    check_tables("no owner at all", 7, iperm7, {plain, no_owner});
    check_tables("owners but no self-collision", 7, iperm7, {plain_body, shares, plain});
    check_tables("a self-colliding sheet only", 7, iperm7, {plain_body, sheet_self});
    check_tables("a self-colliding body only", 7, iperm7, {body_self, plain});
    check_tables("a plain obstacle only", 7, iperm7, {plain});
    check_tables("no meshes", 7, iperm7, {});
    check_tables("n_nodes = 0, one obstacle with side memory", 0, {}, {no_owner});
    check_tables("n_nodes = 0, no meshes", 0, {}, {});
}

int main() {
    form_cases();
    table_cases();
    if (failures) { std::printf("collision_plan: %d check(s) FAILED\n", failures); return 1; }
    std::printf("collision_plan: ok\n");
    return 0;
}
