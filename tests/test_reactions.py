"""Contact and anchor reactions (include/admm_hip.h "contact and anchor reactions"; csrc/reaction.hpp, kernels_reaction.hpp, abi_reaction.inc).

CPU: reaction_query against a numpy.longdouble restatement, its flag and its resultant's documented summation order; the argument and
state errors a host-only context can show.
GPU: what the numbers mean (free particles: f_contact + f_anchor = m (x - x_bar) / dt^2 + the solve's residual, to a rounding bound with
a counted constant), the same bits as the host twin through nine obstacle lists that between them run every collision form 0 .. 7,
the momentum balance of an elastic body, the solver's options (keep_z, a tolerance exit, Anderson acceleration with a rejected
iteration, a released anchor), two shards against one rank, and the C++ class mirror through tests/cpp/reactions.cpp.

The identity.  b = M x_bar + dt^2 sum w^2 (z - u) is the right-hand side of the last solve and A = M + dt^2 sum D^T w^2 D, so
A x - b = M (x - x_bar) - dt^2 sum D^T w^2 (z - u - D x): for the one-node kinds the last sum is the reported f, and
    f_contact + f_anchor = [M (x - x_bar) + (b - A x)] / dt^2
holds whatever the ADMM residual is.  The tests take b from debug_rhs (the device's own vector) and A x from apply_A."""
import threading

import numpy as np
import pytest

from checkers import EPS, KIND, gamma

L = np.longdouble
DT = 0.04
G = np.array([0.0, -9.8, 0.0])
FLOOR, SPHERE, MESH, BOX = 0, 1, 3, 4
FLOOR_Y = 2.0
SPH = [1.5, 2.0, 1.5, 0.25]
W_COLL = 8.0
ERR_ARG, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = 1, 2, 3, 4
# contact_count_kernel counts RX_BLOCK = 128 nodes per block and row_scan_kernel scans RX_SCAN = 64 block counts per pass of its one
# wave: 64 * 128 + 1 collision nodes are one block more than one pass covers (csrc/kernels_reaction.hpp)
RX_BLOCK, RX_SCAN = 128, 64
N_BIG = RX_BLOCK * RX_SCAN + 1
# The constant of the rounding bound C EPS (|b| + |A x| + |M x| + |M x_bar|) / dt^2, by counting roundings, each against a term of the
# bracket (dt^2 w^2 |z - u| <= |b| + |M x_bar| and dt^2 w^2 |x| <= |A x|, so every intermediate below is covered by the bracket):
#   the reported f = w2 * ((z - u) - x): three roundings                                                                         3
#   the device's x_bar = x0 + dt (v0 + dt g): four roundings of intermediates of at most |x0| + dt |v0| + dt^2 |g| <= 1.25 |x_bar|
#     in this scene (the floor sits at y = 2: nothing cancels)                                                                    5
#   M x_bar: one product                                                                                                          1
#   the slot w2h2 * (z - u_new): w2h2 = (dt dt) (w w) carries two roundings more than the w2 of f, the product one               3
#   the right-hand side's gather: 0.0 + slot is exact, + M x_bar rounds once; one more for a second addend's order                2
#   A as assembled (w w, dt dt, their product, + m: the same w2, so three roundings of |A| |x|) and apply_A's product            4
#   the test's own long double evaluation and the conversions of its double inputs                                               1
C_ROUND = 3 + 5 + 1 + 3 + 2 + 4 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _documented_sum(vals):
    """the resultant's summation order as csrc/reaction.hpp states it, in plain Python floats"""
    vals = [float(v) for v in vals]
    nb = (len(vals) + 63) // 64
    part = []
    for b in range(nb):
        a = vals[64 * b:64 * b + 64]
        a += [0.0] * (64 - len(a))
        h = 32
        while h >= 1:
            for i in range(h):
                a[i] = a[i] + a[i + h]
            h //= 2
        part.append(a[0])
    acc = []
    for t in range(256):
        s = 0.0
        for i in range(t, nb, 256):
            s += part[i]
        acc.append(s)
    h = 128
    while h >= 1:
        for t in range(h):
            acc[t] += acc[t + h]
        h //= 2
    return acc[0]


def _documented_resultant(f, point, pivot, flag):
    """{sum f, sum (point - pivot) x f} over the flagged rows in index order: the terms in float64 as reaction.hpp writes them"""
    f, point = f[flag], point[flag]
    r = point - np.asarray(pivot, dtype=np.float64)
    t = [f[:, 0], f[:, 1], f[:, 2], r[:, 1] * f[:, 2] - r[:, 2] * f[:, 1], r[:, 2] * f[:, 0] - r[:, 0] * f[:, 2], r[:, 0] * f[:, 1] - r[:, 1] * f[:, 0]]
    return np.array([_documented_sum(c) for c in t])


def _query_inputs():
    rng = np.random.default_rng(7)
    n = 600
    w2 = rng.uniform(0.5, 100.0, n)
    u = 0.01 * rng.normal(size=(n, 3)); z = rng.normal(size=(n, 3)); x = z + 0.01 * rng.normal(size=(n, 3))
    u[:40] = 0.0                                                          # zero u: depth exactly 0, never a contact
    u[40:80] = rng.choice([1e-310, -3e-320, 5e-324], (40, 3))              # denormal u: its squares underflow
    s = np.repeat(rng.choice([1e-150, 1e150], 60), 3).reshape(60, 3)
    u[80:140] *= 100.0 * s; z[80:140] *= s; x[80:140] *= s
    w2[80:110] = 1e-150; w2[110:140] = 1e150
    nan = np.arange(140, 170)
    u[nan[:10], 0] = np.nan; z[nan[10:20], 1] = np.nan; x[nan[20:], 2] = np.nan
    return w2, u, z, x, nan


def test_reaction_query_against_long_double(pkg):
    """f to the bound of its three operations, depth to the bound of its five (halved by the root) plus the root's own rounding and the
    underflow of the squares; the flag is depth > depth_min on the double value exactly; NaN rows stay NaN and are no contacts"""
    w2, u, z, x, nan = _query_inputs()
    for depth_min in (0.0, 1e-10, 5e-3):
        q = pkg.reaction_query(w2, u, z, x, depth_min=depth_min)
        ok = np.ones(len(w2), bool); ok[nan] = False
        zu = L(z) - L(u)
        f_ld = L(w2)[:, None] * (zu - L(x))
        bound = np.abs(L(w2))[:, None] * (np.abs(zu) * L(EPS) + np.abs(zu - L(x)) * L(gamma(2))) * (1 + L(gamma(3))) + L(2.0) ** -1074
        assert (np.abs(L(q["f"]) - f_ld)[ok] <= bound[ok]).all()
        d_ld = np.sqrt((L(u) ** 2).sum(1))
        d_bound = d_ld * L(0.5 * gamma(5) + EPS) * (1 + L(gamma(5))) + np.sqrt(3 * L(2.0) ** -1074)
        assert (np.abs(L(q["depth"]) - d_ld)[ok] <= d_bound[ok]).all()
        assert (q["depth"][:40] == 0.0).all() and not q["flag"][:40].any()
        assert np.array_equal(q["flag"], q["depth"] > depth_min)
        assert np.isnan(q["depth"][nan[:10]]).all() and not q["flag"][nan[:10]].any()
        assert np.isnan(q["f"][nan]).any(1).all()
        assert q["flag"].sum() > 300


def test_reaction_query_resultant_order(pkg):
    """the resultant equals a plain Python sum in the documented order, bit for bit: fewer contacts than one block, a partial last
    block, and more blocks than the second stage has lanes"""
    rng = np.random.default_rng(11)
    for n in (0, 1, 63, 64, 65, 1000, 64 * 256 + 70):
        w2 = rng.uniform(0.5, 100.0, n)
        u = 0.01 * rng.normal(size=(n, 3)); z = rng.normal(size=(n, 3)); x = z + 0.01 * rng.normal(size=(n, 3))
        u[::5] = 0.0
        pivot = (0.3, -0.2, 0.5)
        q = pkg.reaction_query(w2, u, z, x, depth_min=1e-10, pivot=pivot)
        want = _documented_resultant(q["f"], z, pivot, q["flag"])
        got = np.concatenate([q["force"], q["torque"]])
        assert np.array_equal(got, want), (n, got, want)
        if n >= 63:
            assert q["flag"].sum() >= 0.7 * n and np.abs(got).min() > 0.0


def _p(a):
    import ctypes as C
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def test_reaction_query_argument_checks(pkg):
    lib = pkg.lib()
    a = np.zeros((2, 3)); w = np.ones(2); r6 = np.zeros(6)
    call = lambda n, w2, u, z, x, dm: lib.admm_hip_reaction_query(n, _p(w2), _p(u), _p(z), _p(x), dm, None, None, None, None, _p(r6))
    assert call(2, w, a, a, a, 0.0) == 0 and call(0, None, None, None, None, 0.0) == 0
    assert call(-1, w, a, a, a, 0.0) == ERR_ARG
    for dm in (-1e-300, -1.0, float("nan")):
        assert call(2, w, a, a, a, dm) == ERR_ARG
    for k in range(4):
        args = [w, a, a, a]; args[k] = None
        assert call(2, *args, 0.0) == ERR_ARG
    with pytest.raises(pkg.AdmmHipError):
        pkg.reaction_query(w, a, a, a, depth_min=-1.0)


def _host_only_bar(pkg):
    s = pkg.make_bar_system(2, 2, 3, device_id=-1)
    s.coll = s.add_forces(KIND["COLLISION"], np.arange(s.n_nodes, dtype=np.int32), [W_COLL])
    s.set_collision_shapes([FLOOR], [[0.0, -1.0, 0.0, 0.0]])
    return s


def _code(pkg, fn, *a, **k):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*a, **k)
    return int(str(e.value).split("error ")[1].split(":")[0])


def test_argument_and_state_errors_on_the_host(pkg):
    """the checks in the order include/admm_hip.h states: the call's own arguments first (a batch of another kind: UNSUPPORTED, a
    negative depth_min: ARG), then the host-only context, refused like every compute call"""
    s = _host_only_bar(pkg)
    s.initialize()
    assert _code(pkg, s.batch_reaction, 0) == ERR_UNSUPPORTED                # the tet batch
    assert _code(pkg, s.contacts, depth_min=-1.0) == ERR_ARG
    assert _code(pkg, s.contacts, depth_min=float("nan")) == ERR_ARG
    assert _code(pkg, s.contact_resultant, depth_min=-1e-300) == ERR_ARG
    assert s.L.admm_hip_batch_reaction(s.h, 99, None, None) == ERR_ARG and s.L.admm_hip_batch_reaction(s.h, -1, None, None) == ERR_ARG
    assert s.L.admm_hip_get_contacts(s.h, 0.0, None, 4, None) == ERR_ARG        # a capacity without records
    for fn, a in ((s.batch_reaction, (1,)), (s.batch_reaction, (s.coll,)), (s.node_reactions, ()), (s.contacts, ()), (s.contact_resultant, ())):
        assert _code(pkg, fn, *a) == ERR_HIP
    assert s.L.admm_hip_node_reactions(None, None, None, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 1: what the numbers mean, on free particles
# ---------------------------------------------------------------------------------------------------------------------------------
def _particles(pkg, N, mode="mixed", n_anchor=3, sphere=True):
    """N massed nodes, no elastic force, one COLLISION batch over all of them, a floor at y = 2 and (`sphere`) a sphere half sunk in it, gravity;
    odd nodes (mode "all": all, "none": none) start 0.02 .. 0.1 above the floor at 5 m/s downwards and hit it within the frame, the
    others hang 0.6 above it; n_anchor more nodes of their own carry one ANCHOR element each, the target 0.05 above the node"""
    rng = np.random.default_rng(1000 + N)
    hit = {"mixed": np.arange(N) % 2 == 1, "all": np.ones(N, bool), "none": np.zeros(N, bool)}[mode]
    x0 = np.stack([rng.uniform(1.0, 2.0, N), np.where(hit, FLOOR_Y + rng.uniform(0.02, 0.1, N), FLOOR_Y + rng.uniform(0.6, 0.9, N)), rng.uniform(1.0, 2.0, N)], 1)
    v0 = np.stack([rng.uniform(-0.2, 0.2, N), np.where(hit, -5.0, 0.0), rng.uniform(-0.2, 0.2, N)], 1)
    xa = np.stack([1.2 + 0.2 * np.arange(n_anchor), np.full(n_anchor, 3.0), np.full(n_anchor, 1.5)], 1)
    x0 = np.concatenate([x0, xa]); v0 = np.concatenate([v0, np.zeros((n_anchor, 3))])
    m = rng.uniform(0.5, 2.0, N + n_anchor)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x0.ravel(), np.repeat(m, 3))
    s.coll = s.add_forces(KIND["COLLISION"], np.arange(N, dtype=np.int32), [W_COLL])
    s.anch = s.add_forces(KIND["ANCHOR"], np.arange(N, N + n_anchor, dtype=np.int32), [-1.0, 1.0], targets=xa + [0.0, 0.05, 0.0])
    s.add_gravity(G)
    s.set_collision_shapes([FLOOR, SPHERE][:2 if sphere else 1], [[0.0, FLOOR_Y, 0.0, 0.0], SPH][:2 if sphere else 1])
    s.initialize()
    s.m_v = v0.ravel()
    s.N, s.x0, s.v0, s.m = N, x0, v0, m
    return s


def _identity(s, x0=None, v0=None, label=""):
    """asserts f_contact + f_anchor = [M (x - x_bar) + (b - A x)] / dt^2 per entry within C_ROUND EPS (|b| + |A x| + |M x| + |M x_bar|) / dt^2
    after the step that just ran from (x0, v0); -> (f_contact, f_anchor, info, the largest ratio to the bound)"""
    x0 = s.x0 if x0 is None else x0
    v0 = s.v0 if v0 is None else v0
    x = s.m_x.reshape(-1, 3)
    b = s.debug_rhs().reshape(-1, 3)
    Ax = s.apply_A(x).reshape(-1, 3)
    fc, fa, info = s.node_reactions()
    dt, m = L(DT), L(s.m)[:, None]
    xbar = L(x0) + dt * (L(v0) + dt * L(G))
    want = (m * (L(x) - xbar) + (L(b) - L(Ax))) / (dt * dt)
    scale = (np.abs(L(b)) + np.abs(L(Ax)) + m * np.abs(L(x)) + m * np.abs(xbar)) / (dt * dt)
    assert (np.abs(L(b) - L(Ax)) <= 1e-9 * np.abs(L(b))).all()              # b is the vector the last solve was handed
    err = np.abs(L(fc) + L(fa) - want)
    ratio = float((err / (C_ROUND * L(EPS) * scale)).max())
    print("reaction identity %s: %d nodes, max error / bound = %.3f (C = %d)" % (label, len(x), ratio, C_ROUND))
    assert ratio <= 1.0, ratio
    return fc, fa, info, ratio


def _dense_contacts(pkg, s, depth_min):
    """the contact list from the dense outputs, filtered on the host -> a structured array like System.contacts'"""
    fc, _, _ = s.node_reactions()
    f_el, depth = s.batch_reaction(s.coll)
    z = s.read_local(s.coll)["z"]
    assert np.array_equal(fc[:s.N], f_el) and not fc[s.N:].any()             # one collision element per node, in node order
    k = np.flatnonzero(depth > depth_min)
    rec = np.zeros(len(k), pkg.CONTACT_DTYPE)
    rec["node"], rec["f"], rec["point"], rec["depth"] = k, f_el[k], z[k], depth[k]
    return rec


def _same_records(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("node", "f", "point", "depth"))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, N_BIG])
def test_reactions_balance_the_momentum_of_free_particles(pkg, N):
    """one step(10): the identity per node and component; the nodes that hit report a contact with an upward force, the others none at
    the default threshold; the compact list is the dense output filtered on the host, in ascending node order, the same bits; the
    anchors pull upwards.  N_BIG: one more count block than one pass of the scan covers."""
    s = _particles(pkg, N)
    s.step(10)
    fc, fa, info, _ = _identity(s, label="N = %d" % N)
    assert info == dict(batches_collision=1, batches_anchor=1, batches_skipped=0, n_contacts=info["n_contacts"])
    hit = np.flatnonzero(np.arange(N) % 2 == 1)
    c = s.contacts()
    assert np.array_equal(c["node"], hit) and (c["f"][:, 1] > 0).all() and (c["depth"] > 1e-3).all()
    assert (c["point"][:, 1] >= FLOOR_Y).all()
    for dm in (0.0, 1e-10, 0.05):
        want = _dense_contacts(pkg, s, dm)
        got = s.contacts(depth_min=dm)
        assert _same_records(got, want), dm
        assert s.last_contact_count == len(want)
        if dm == 0.0:
            assert info["n_contacts"] == len(want)
    assert (fa[N:, 1] > 0).all() and not fa[:N].any()
    f_a, d_a = s.batch_reaction(s.anch)
    assert np.array_equal(f_a, fa[N:]) and (d_a > 0).all()
    # the resultant: the host twin on the same rows, bit for bit
    w2 = s.read_rest(s.coll)["weight"] ** 2
    r = s.read_local(s.coll)
    pivot = (1.5, 2.0, 1.5)
    q = pkg.reaction_query(w2, r["u"], r["z"], s.m_x.reshape(-1, 3)[:N], pivot=pivot)
    force, torque, count = s.contact_resultant(pivot=pivot)
    assert count == len(c) and np.array_equal(force, q["force"]) and np.array_equal(torque, q["torque"])
    if len(c):
        assert force[1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["all", "none"])
def test_all_or_no_node_in_contact_and_capacities(pkg, mode):
    """every node in contact, no node in contact; capacity 0, count - 1 and count: the first `capacity` records and the true count"""
    N = 65
    s = _particles(pkg, N, mode)
    s.step(10)
    _identity(s, label=mode)
    full = s.contacts()
    count = N if mode == "all" else 0
    assert len(full) == count and s.last_contact_count == count and _same_records(full, _dense_contacts(pkg, s, 1e-10))
    for cap in sorted({0, max(count - 1, 0), count}):
        part = s.contacts(capacity=cap)
        assert s.last_contact_count == count and _same_records(part, full[:min(cap, count)]), cap
    force, torque, n = s.contact_resultant()
    assert n == count
    if mode == "none":
        assert not force.any() and not torque.any()
    else:
        assert force[1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 64, 65, 64 * 256 + 1])
def test_contact_resultant_on_the_one_row_path(pkg, count):
    """contact_resultant sums all contacts as ONE row of the per-entry sums (entry_partial_kernel without a permutation, then
    entry_reduce_kernel over the ceil(count / 64) partials that are filled).  Contact counts (asserted) of no block, one contact, one full
    block, a block and one, and 64 * 256 + 1: 257 partials, so thread 0 of the second stage adds two.  `count` nodes that all hit the
    floor (three that do not at count 0), one frame, on two fresh systems.  Attribution off -- the call needs none of its buffers: bit for
    bit the host twin reaction_query.  Attribution on: the twin again, and entry_resultants summed over its rows.  The list is the floor
    alone, so every contact is owned by entry 0 (asserted) and row 0 goes through the permutation, which is then the identity; the row
    of the contacts nobody owns is empty, +0.0 six times, so the rows' sum is row 0 + 0.0 and must be contact_resultant's bits."""
    pivot = (1.5, 2.0, 1.5)
    for attribution in (False, True):
        s = _particles(pkg, count if count else 3, "all" if count else "none", sphere=False)
        if attribution:
            s.enable_contact_attribution()
        s.step(10)
        r = s.read_local(s.coll)
        q = pkg.reaction_query(s.read_rest(s.coll)["weight"] ** 2, r["u"], r["z"], s.m_x.reshape(-1, 3)[:s.N], pivot=pivot)
        force, torque, n = s.contact_resultant(pivot=pivot)
        assert n == count == int(q["flag"].sum())
        assert np.array_equal(force, q["force"]) and np.array_equal(torque, q["torque"]), (count, attribution)
        assert force[1] > 0 if count else not (force.any() or torque.any())
        if attribution:
            ef, et, ec = s.entry_resultants(pivot=pivot)
            assert ec.tolist() == [count, 0]
            assert np.array_equal(ef[0] + ef[1], force) and np.array_equal(et[0] + et[1], torque), (count, ef, et)


@pytest.mark.gpu
def test_call_before_any_step_is_a_state_error(pkg):
    s = _particles(pkg, 5)
    for fn, a in ((s.batch_reaction, (s.coll,)), (s.node_reactions, ()), (s.contacts, ()), (s.contact_resultant, ())):
        assert _code(pkg, fn, *a) == ERR_STATE
    s.step(2)
    assert s.node_reactions()[2]["batches_collision"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the host twin's bits through every kind of list
# ---------------------------------------------------------------------------------------------------------------------------------
H = 0.05
DIMS = (2, 2, 3)


def _bar_scene(pkg, kind, device_id=0, anchors=False, shard=None, tet=("TET_NH", [1e5, 1e5, 5])):
    """the 2 x 2 x 3 bar (h = 0.05, its lowest nodes at y = 0; Neo-Hookean unless `tet` says otherwise), one collision element per bar
    node, gravity, resting on and against one obstacle list -> (system, the form its collision batch must run).  kind "sheet" adds a
    3 x 3-node cloth patch far from the bar whose surface collides with itself and sits in the list behind the floor."""
    mg = pkg.meshgen
    x, tets = mg.bar(*DIMS, H)
    n = len(x)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=device_id)
    s.set_timestep(DT)
    s.n_elastic = 1
    if kind == "sheet":
        from test_collision_shell import _grid
        V5, F5 = _grid(2)
        s.add_nodes(np.concatenate([x, V5 + [50.0, 0.0, 0.0]]).ravel(), np.repeat(np.concatenate([m, np.full(len(V5), 0.01)]), 3))
    else:
        s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.tets = s.add_forces(KIND[tet[0]], tets, tet[1])
    if kind == "sheet":
        s.add_forces(KIND["TRI_STRAIN"], F5 + n, [100.0, 0.95, 1.05, 1.0])
        s.n_elastic = 2
    s.coll = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W_COLL])
    if anchors:
        top = np.flatnonzero(x[:, 1] == x[:, 1].max())[:2].astype(np.int32)
        s.anch = s.add_forces(KIND["ANCHOR"], top, [-1.0, 1.0])
    s.add_gravity(G)
    lo, hi = x.min(0), x.max(0)
    c = 0.5 * (lo + hi)
    y0 = lo[1] + 0.004                                                     # the obstacle's top: the bar's lowest layer starts 4 mm inside it
    form = 0
    if kind in ("floor", "friction", "moving"):
        s.set_collision_shapes([FLOOR], [[0.0, y0, 0.0, 0.0]])
        if kind != "floor":
            s.set_collision_friction([0.5]); form = 1
        if kind == "moving":                                               # a conveyor: the floor slides under the bar
            s.set_collision_motion([[0.2, 0.0, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]); form = 2
    elif kind == "sheet":
        mid = s.add_sheet_surface(n, len(V5), F5 + n, 0.05, self_collision=True)
        s.set_collision_shapes([FLOOR, MESH], [[0.0, y0, 0.0, 0.0], [0.0, 0.0, 0.0, mid]])
        form = 5
    elif kind == "mesh":
        from test_collision_shell import _cube
        V, F = _cube()
        mid = s.add_collision_mesh(0.4 * V, F)                            # a cube of edge 0.4 whose top face is at y0
        s.set_collision_shapes([MESH], [[c[0], y0 - 0.2, c[2], mid]])
    elif kind in ("shell", "shell_memory"):
        from test_collision_shell import _grid
        V, F = _grid(4, 0.6)
        mid = s.add_collision_mesh(pkg.Mesh(V, F, 0.01), None)            # a sheet of half thickness 0.01 whose upper face is at y0
        form = 4
        if kind == "shell_memory":
            s.set_collision_mesh_side_memory(mid, 0.05); form = 6
        s.set_collision_shapes([MESH], [[c[0], y0 - 0.01, c[2], mid]])
    elif kind == "box":
        from test_collision_frames import _frame, _rot
        s.set_collision_shapes([BOX], [[0.3, 0.1, 0.3, 0.0]])
        s.set_collision_frames([_frame(_rot([0.0, 1.0, 0.0], 0.4), [c[0], y0 - 0.1, c[2]])])      # turned about the vertical: its top stays at y0
        form = 3
    else:
        assert kind == "body"
        mid = s.add_body_surface(0, n, mg.tet_surface(tets), self_collision=(0.005, 0.01, 0.03))
        s.set_collision_shapes([FLOOR, MESH], [[0.0, y0, 0.0, 0.0], [0.0, 0.0, 0.0, mid]])
        form = 7
    if shard is None:
        s.initialize()
    else:                                                                  # (a rank of a sharded run: initialized together with the others)
        s.set_shard(*shard); s.set_shard_mode("subtree")
    s.N, s.x0, s.m = n, x, m
    return s, form


# the six lists the scenes are named after run forms 0, 0, 6, 1, 3 and 7; "moving", "shell" and "sheet" add the forms 2, 4 and 5
BAR_KINDS = ["floor", "mesh", "shell_memory", "friction", "box", "body", "moving", "shell", "sheet"]
BAR_FORMS = dict(floor=0, mesh=0, shell_memory=6, friction=1, box=3, body=7, moving=2, shell=4, sheet=5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", BAR_KINDS)
def test_same_bits_as_the_host_twin(pkg, kind):
    """every collision form 0 .. 7 (asserted): three frames of step(10) on each list and, after every frame, batch_reaction,
    node_reactions, contacts and contact_resultant against reaction_query fed read_local's u and z and m_x, bit for bit; in at least one
    frame the obstacle carries the bar (a contact, the resultant upwards; the first frame starts with the lowest layer inside it); the
    run is unchanged by the calls: x after two more frames is bitwise that of a twin that never asked, and the frame graph went on being
    replayed"""
    s, form = _bar_scene(pkg, kind)
    twin, _ = _bar_scene(pkg, kind)
    assert s.collision_form() == form == BAR_FORMS[kind]
    N = s.N
    w2 = s.read_rest(s.coll)["weight"] ** 2
    pivot = (0.05, 0.0, 0.075)
    carried = []
    for frame in range(3):
        s.step(10); twin.step(10)
        launches = s.graph_state()
        r = s.read_local(s.coll)
        x = s.m_x.reshape(-1, 3)[:N]
        for dm in (1e-10, 1e-4):
            q = pkg.reaction_query(w2, r["u"], r["z"], x, depth_min=dm, pivot=pivot)
            f, depth = s.batch_reaction(s.coll)
            assert np.array_equal(f, q["f"]) and np.array_equal(depth, q["depth"])
            fc, fa, info = s.node_reactions()
            assert np.array_equal(fc[:N], q["f"]) and not fc[N:].any() and not fa.any()
            assert info["batches_collision"] == 1 and info["batches_anchor"] == 0 and info["batches_skipped"] == s.n_elastic
            c = s.contacts(depth_min=dm)
            k = np.flatnonzero(q["flag"])
            assert np.array_equal(c["node"], k) and np.array_equal(c["f"], q["f"][k]) and np.array_equal(c["point"], r["z"][k]) and np.array_equal(c["depth"], q["depth"][k])
            force, torque, count = s.contact_resultant(pivot=pivot, depth_min=dm)
            assert count == len(k) and np.array_equal(force, q["force"]) and np.array_equal(torque, q["torque"])
        carried.append((len(k), float(force[1])))
        assert np.array_equal(s.read_local(s.coll)["u"], r["u"]) and np.array_equal(s.read_local(s.coll)["z"], r["z"])
    print("%s: contacts and vertical resultant per frame: %s" % (kind, carried))
    assert any(n >= 1 and fy > 0 for n, fy in carried), (kind, carried)
    for _ in range(2):
        s.step(10); twin.step(10)
    assert np.array_equal(s.m_x, twin.m_x) and np.array_equal(s.m_v, twin.m_v)
    after = s.graph_state()
    assert after == twin.graph_state() and after["graph_launches"] > launches["graph_launches"], (launches, after)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 3: momentum balance on an elastic body
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_momentum_balance_on_an_elastic_body(pkg):
    """the bar dropped on a floor with two anchored corners, Neo-Hookean, not converged (step(5)): the elastic selectors are
    translation-invariant, so their node shares sum to zero and, per axis,
        sum_nodes (f_contact + f_anchor) = sum_nodes [M (x - x_bar) + (b - A x)] / dt^2
    to the rounding bound of the particle test, C_ROUND EPS (|b| + |A x| + |M x| + |M x_bar|) / dt^2, summed over the nodes.  At least
    one contact, and the vertical resultant is positive."""
    s, _ = _bar_scene(pkg, "floor", anchors=True)
    v0 = np.zeros_like(s.x0); v0[:, 1] = -0.5
    s.m_v = v0.ravel()
    s.step(5)
    x = s.m_x.reshape(-1, 3)
    b = s.debug_rhs().reshape(-1, 3)
    Ax = s.apply_A(x).reshape(-1, 3)
    fc, fa, info = s.node_reactions()
    assert info["batches_skipped"] == 1 and info["n_contacts"] >= 1
    dt, m = L(DT), L(s.m)[:, None]
    xbar = L(s.x0) + dt * (L(v0) + dt * L(G))
    want = ((m * (L(x) - xbar) + (L(b) - L(Ax))) / (dt * dt)).sum(0)
    scale = ((np.abs(L(b)) + np.abs(L(Ax)) + m * np.abs(L(x)) + m * np.abs(xbar)) / (dt * dt)).sum(0)
    got = (L(fc) + L(fa)).sum(0)
    ratio = np.abs(got - want) / (C_ROUND * L(EPS) * scale)
    print("momentum balance: per-axis error / bound =", [float(v) for v in ratio])
    assert (ratio <= 1.0).all(), ratio
    force, _, count = s.contact_resultant()
    assert count >= 1 and force[1] > 0 and len(s.contacts()) == count


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 4: options
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("option", ["keep_z_off", "tolerance", "acceleration", "released_anchor"])
def test_identity_under_the_solvers_options(pkg, option):
    """the particle identity (N = 65) with admm_hip_keep_z(ctx, 0) (the collision and anchor kernels store z regardless), with a
    tolerance that ends the loop early (fewer iterations than the cap ran), with Anderson acceleration at window 3 (every iteration
    writes its s_out to the batches' z and u and rebuilds the shares before the solve: abi_anderson.inc, abi_step.inc), and with a
    released anchor, which goes through the same formula (its u is rounding residue, its f the last iteration's increment)"""
    N = 65
    s = _particles(pkg, N)
    cap = 10
    if option == "keep_z_off":
        s.keep_z(False)
    elif option == "tolerance":
        # a tolerance every residual meets, tested at every third iteration: the loop ends after three of ten, far from converged (in this scene,
        # where some nodes are inside the sphere and under the floor at once, |r| and |s| were still above 1 after 400 iterations)
        s.set_tolerance(1e300, 1e300, 3)
    elif option == "acceleration":
        s.set_acceleration(3)
    else:
        s.update_anchors(s.anch, active=[1, 0, 1])
    s.step(cap)
    fc, fa, info, _ = _identity(s, label=option)
    assert len(s.contacts()) == 32
    if option == "tolerance":
        ran = s.residuals()[2]
        assert ran == 3 < cap, ran
    if option == "acceleration":
        log = s.acceleration_log()
        print("acceleration: accepted %s, extrapolated %s" % ("".join(str(int(r["accepted"])) for r in log), "".join(str(int(r["extrapolated"])) for r in log)))
        # an extrapolated iterate, and a rejected one before the last (the reset restores s_def into z and u): both reach the last solve
        assert len(log) == cap and any(r["extrapolated"] for r in log) and any(not r["accepted"] for r in log[:-1])
    if option == "released_anchor":                                        # the same formula, no special case: the host twin's bits
        r = s.read_local(s.anch)
        q = pkg.reaction_query(s.read_rest(s.anch)["weight"] ** 2, r["u"], r["z"], s.m_x.reshape(-1, 3)[N:])
        assert np.array_equal(fa[N:], q["f"]) and np.array_equal(s.batch_reaction(s.anch)[1], q["depth"])
        assert np.abs(r["u"][1]).max() <= 64 * EPS * np.abs(s.x0[N + 1]).max() < np.abs(r["u"][0]).max()      # its u is rounding residue, the held ones' is not


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 5: shards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards_add_up_to_one_rank(pkg, monkeypatch):
    """two contexts on one GPU (one thread each, as tests/test_sharding.py starts them): the ranks' node_reactions add up to the
    one-rank vectors.  The sharding tests hold x to 1e-9 over frames for scenes whose local step is exact (cloth, corotational tets; a
    Neo-Hookean or StVK bar, whose truncated L-BFGS amplifies the order of the sums, is held to 1e-5 there), so the bar is corotational
    here (TET_LINEAR).  f = w^2 ((z - u) - x): each output is bound by 1e-9 times the w^2 of its own batch, W_COLL^2 = 64 for f_contact
    and the anchors' 1000^2 for f_anchor, no other factor."""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "8")
    tet = ("TET_LINEAR", [1e5])
    one, _ = _bar_scene(pkg, "floor", anchors=True, tet=tet)
    world = 2
    shards = [_bar_scene(pkg, "floor", anchors=True, shard=(r, world), tet=tet)[0] for r in range(world)]
    for sh, hk in zip(shards, _thread_allreduce_hooks(world)):
        sh.set_allreduce(hk)
    pkg.initialize_together(shards)
    one.step(10)
    out, errs = [None] * world, []

    def run(r):
        try:
            shards[r].step(10)
            out[r] = shards[r].node_reactions()
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    fc1, fa1, info1 = one.node_reactions()
    tol_c = 1e-9 * (one.read_rest(one.coll)["weight"] ** 2).max()
    tol_a = 1e-9 * (one.read_rest(one.anch)["weight"] ** 2).max()
    assert tol_c == 1e-9 * W_COLL ** 2
    fc = sum(o[0] for o in out); fa = sum(o[1] for o in out)
    print("shards: |f_contact| error %.3g (bound %.3g), |f_anchor| error %.3g (bound %.3g), |x| error %.3g" %
          (np.abs(fc - fc1).max(), tol_c, np.abs(fa - fa1).max(), tol_a, max(np.abs(sh.m_x - one.m_x).max() for sh in shards)))
    assert np.abs(fc - fc1).max() <= tol_c and np.abs(fa - fa1).max() <= tol_a
    assert np.abs(fc1).max() > 10 * tol_c and np.abs(fa1).max() > 10 * tol_a      # the forces are well above the bounds: zeros would not pass
    assert sum(o[2]["n_contacts"] for o in out) == info1["n_contacts"] >= 1
    assert sorted(np.concatenate([s.local_elements(one.coll) for s in shards]).tolist()) == list(range(one.N))
    assert min(s.local_elements(one.anch).size for s in shards) == 0      # one rank holds no anchor: an empty batch went through its gather


# ---------------------------------------------------------------------------------------------------------------------------------
# the C++ class mirror (host/admm/System.hpp): tests/cpp/reactions.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    import os
    assert os.path.exists(compile_cpp("reactions", pkg))


@pytest.mark.gpu
def test_cpp_mirror_reports_reactions(pkg):
    """System::node_reactions, contacts and contact_resultant on three unit-mass nodes (one dropped on a floor, one free, one anchored):
    refused before the first step (the program checks it), then one contact, node 0, pushed upwards from a point on the floor; its
    record is the node's f_contact; the resultant about (1, 0, 0) is that one force and its torque, in reaction.hpp's operations; the
    anchor holds its node against gravity; the dropped node obeys f = m (x - x_bar) / dt^2 (a 3 x 3 diagonal system, solved exactly up
    to rounding: 1e-9 relative is far above it)"""
    import subprocess
    from test_cpp_host import compile_cpp
    r = subprocess.run([compile_cpp("reactions", pkg)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr)
    def numbers(text):                                                      # the labels between the figures are skipped
        out = []
        for tok in text.split():
            try:
                out.append(float(tok))
            except ValueError:
                pass
        return out
    rows = {}
    for line in r.stdout.splitlines():
        key, rest = line.split(":", 1)
        rows.setdefault(key, []).append(numbers(rest))
    assert rows["info"] == [[1.0, 1.0, 0.0, rows["info"][0][3]]] and rows["info"][0][3] >= 1
    nodes = np.array(rows["node"])                                           # index, x[3], contact[3], anchor[3]
    x, fc, fa = nodes[:, 1:4], nodes[:, 4:7], nodes[:, 7:10]
    assert len(rows["contact"]) == 1
    c = np.array(rows["contact"][0])                                         # node, f[3], point[3], depth
    assert c[0] == 0 and np.array_equal(c[1:4], fc[0]) and c[2] > 0 and c[5] >= 0.0 and c[7] > 1e-3
    res = np.array(rows["resultant"][0])
    rr = c[4:7] - np.array([1.0, 0.0, 0.0])
    torque = np.array([rr[1] * c[3] - rr[2] * c[2], rr[2] * c[1] - rr[0] * c[3], rr[0] * c[2] - rr[1] * c[1]])
    assert res[0] == 1 and np.array_equal(res[1:4], c[1:4]) and np.array_equal(res[4:7], torque)
    assert fa[2, 1] > 0 and not fa[:2].any()
    xbar_y = 0.05 + DT * (-5.0 + DT * G[1])
    want = (x[0, 1] - xbar_y) / DT ** 2
    assert abs(fc[0, 1] - want) <= 1e-9 * abs(want), (fc[0, 1], want)
