"""User-defined forces (generic batches: admm_hip_add_generic_batch + the project hook) on general selector rows and across shards.

Every other test of this path uses rows of at most two +-1 entries, where each (node, component) slot is fed by one row.  Here:

  1. the built-in arithmetic restated as user forces (one GPU): the oracle's own selector rows (D_triplets, wdiag) of TET_NH,
     TET_VOLUME, TRI_STRAIN, BEND and TET_LINEAR elements -- 3 to 9 rows per node slot, coefficients of any value -- given shuffled and
     with entries split into duplicates, projected in the hook by orc_force_project on a second oracle (the hyperelastic warm start).
     D_i x and the local step bitwise; one ADMM iteration against the oracle and the built-in batch; residuals per iteration;
     set_weights + recompute_weights on a generic batch.  Dense path and panel sweeps, both slot layouts.
  2. irregular user rows (empty rows, an element without rows, weights that differ inside one element, a centroid over 50 nodes with
     coefficients 1/k, a node fed by two generic batches and a built-in one) against an extended-precision reference built from the
     explicit triplets (checkers.SparseReference.from_selector).
  3. elements whose nodes lie in two ranks' subtrees: subtree sharding refuses them at initialize (CPU: host-only contexts; GPU:
     every rank alike), contiguous sharding runs them and agrees with the one-rank run.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import checkers
from checkers import KIND, KIND_ROWS, Oracle, SparseReference

DT = 0.04
GRAVITY = (0.0, -9.8, 0.0)
FWD_TOL, KAPPA_BASE, BWD_ERR_TOL = 1e-12, 2e4, 1e-14      # the bounds of test_wide_supernodes.py


def fwd_tol(kappa1):
    return FWD_TOL * max(1.0, kappa1 / KAPPA_BASE)


# ---------------------------------------------------------------- scenes ----
class Scene:
    """nodes, masses and a list of (kind name, index array, params, restate as a user force?) in add order"""

    def __init__(self, name, x, m3, forces, dt=DT, iters=1):
        self.name, self.x, self.m3, self.forces, self.dt, self.iters = name, np.asarray(x, dtype=np.float64), m3, forces, dt, iters

    def oracle(self, iters=1):
        o = Oracle(); o.settings(self.dt, iters)
        o.add_nodes(self.x.ravel(), self.m3)
        for kind, idx, par, _ in self.forces:
            o.add_forces(KIND[kind], idx, par)
        o.add_gravity(GRAVITY)
        assert o.initialize()
        return o

    def first_force(self):
        f, out = 0, []
        for kind, idx, par, _ in self.forces:
            out.append(f); f += np.asarray(idx).reshape(-1, checkers.KIND_NODES[KIND[kind]]).shape[0]
        return out


def bar_scene(pkg):
    """a Neo-Hookean / volume-preserving bar: TET_VOLUME built-in, TET_NH and TET_VOLUME as user forces, anchors built-in"""
    mg = pkg.meshgen
    x, t = mg.bar(3, 3, 10)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    a, b = t.shape[0] // 3, 2 * t.shape[0] // 3
    return Scene("bar", x, m3, [("TET_VOLUME", t[:a], [100.0, 0.9, 1.1], False), ("TET_NH", t[a:b], [1e5, 1e5, 5], True),
                                ("TET_VOLUME", t[b:], [3e3, 0.95, 1.05], True), ("ANCHOR", mg.bar_anchor_nodes(3, 3), [-1.0, 1.0], False)])


def cloth_scene(pkg):
    """a cloth with hinges hanging from two corners: triangle strain and bend as user forces"""
    mg = pkg.meshgen
    w = 14
    x, tris = mg.sym_plane(w, w, size=1.0)
    hinges = mg.bend_hinges(tris)
    m3 = np.full(x.size, 0.5 / x.shape[0])
    return Scene("cloth", x, m3, [("TRI_STRAIN", tris, [100.0, 0.95, 1.05, 1.0], True), ("BEND", hinges, [20.0], True),
                                  ("ANCHOR", np.array([0, w], np.int32), [-1.0, 1.0], False)], iters=6)


def delaunay_scene(pkg):
    """Delaunay tets of random points (irregular valence): corotational tets as user forces"""
    x, m3, forces = checkers.delaunay_scene(600, seed=11, box=(0.5, 0.5, 2.0))
    (k1, t, p1), (k2, an, p2) = forces
    return Scene("delaunay", x, m3, [(k1, t, p1, True), (k2, an, p2, False)], iters=6)


SCENES = {"bar": bar_scene, "cloth": cloth_scene, "delaunay": delaunay_scene}


class RestatedHook:
    """project() of the generic batches that restate oracle forces: element e of a run is the oracle's force f0 + e, projected with
    orc_force_project on `oracle` (an instance of its own, which carries the warm start of the hyperelastic forces).  Records D_i x."""

    def __init__(self, s, oracle, runs):
        self.s, self.o, self.runs, self.dx, self.ids = s, oracle, runs, [], {}

    def __call__(self, dt, Dx, u, z):
        self.dx.append(Dx.copy())
        lib, dp = self.o.lib, C.POINTER(C.c_double)
        for b, f0, erp, g0, _ in self.runs:
            ids = self.ids.setdefault(b, self.s.local_elements(b))
            for e in ids:
                g = 8 * (g0 + int(erp[e]))
                lib.orc_force_project(lib.orc_get_force(self.o.h, f0 + int(e)), dt, C.cast(Dx.ctypes.data + g, dp), C.cast(u.ctypes.data + g, dp),
                                      C.cast(z.ctypes.data + g, dp))


def build_system(pkg, scene, restate=True, seed=0, device_id=0):
    """the scene as a System, the marked batches as generic batches (triplets shuffled, a third of them split into halves) and the
    hook on a fresh oracle; -> (system, hook or None, runs: (batch, first force, elem_row_ptr, first generic row, oracle rows))"""
    s = pkg.System(device_id=device_id); s.set_timestep(scene.dt)
    s.add_nodes(scene.x.ravel(), scene.m3)
    rng = np.random.default_rng(seed)
    oh = scene.oracle() if restate else None
    runs, g0 = [], 0
    for (kind, idx, par, user), f0 in zip(scene.forces, scene.first_force()):
        n = np.asarray(idx).reshape(-1, checkers.KIND_NODES[KIND[kind]]).shape[0]
        if restate and user:
            erp, tr, tc, tv, w, orows = checkers.selector_rows(oh, f0, f0 + n, rng, split=0.3)
            b = s.add_generic(erp, tr, tc, tv, w)
            runs.append((b, f0, erp, g0, orows)); g0 += int(erp[-1])
        else:
            s.add_forces(KIND[kind], idx, par)
    s.add_gravity(GRAVITY)
    hook = None
    if runs:
        hook = RestatedHook(s, oh, runs)
        s.set_project_hook(hook)
    return s, hook, runs


def dx_reference(o, xcur):
    """D x in the oracle's rows, entries in ascending column order from 0.0 (Oracle.local_step's order)"""
    rr, cc, vv = o.D_triplets()
    k = np.lexsort((cc, rr))
    Dx = np.zeros(o.rows)
    for r_, c_, v_ in zip(rr[k].tolist(), cc[k].tolist(), vv[k].tolist()):
        Dx[r_] += v_ * xcur[c_]
    return Dx


def multi_row_slots(scene, runs):
    """the largest number of rows of one user force that feed one (node, component) slot"""
    o = scene.oracle()
    rr, cc, _ = o.D_triplets()
    best = 0
    for _, f0, erp, _, orows in runs:
        force_of = np.repeat(np.arange(f0, f0 + erp.size - 1), np.diff(erp))
        sel = np.isin(rr, orows)
        fo = np.zeros(o.rows, np.int64); fo[orows] = force_of
        key = fo[rr[sel]] * (3 * scene.x.shape[0]) + cc[sel]
        best = max(best, int(np.unique(key, return_counts=True)[1].max()))
    return best


def close_residuals(r, s, ro, so):
    """|r| and |s| of every iteration within 1e-10 of the oracle's, relative to each value and, for values at the rounding floor
    (|s| of a first iteration that barely moves z), to the frame's largest residual"""
    floor = 1e-10 * max(np.abs(ro).max(), np.abs(so).max())
    assert np.all(np.abs(r - ro) <= 1e-10 * np.abs(ro) + floor), ("|r|", r, ro)
    assert np.all(np.abs(s - so) <= 1e-10 * np.abs(so) + floor), ("|s|", s, so)


def set_path(monkeypatch, path, layout):
    monkeypatch.delenv("ADMM_HIP_DENSE_MAX", raising=False)
    if path == "panels":
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.delenv("ADMM_HIP_SLOTS_NODE_SORTED", raising=False)
    if layout == "node_sorted":
        monkeypatch.setenv("ADMM_HIP_SLOTS_NODE_SORTED", "1")


# ---------------------------------------------------------------- 1. built-in arithmetic restated as user forces ----
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rank_major", "node_sorted"])
@pytest.mark.parametrize("path", ["dense", "panels"])
@pytest.mark.parametrize("name", ["bar", "cloth", "delaunay"])
def test_builtin_forces_restated_as_user_forces(pkg, monkeypatch, name, path, layout):
    scene = SCENES[name](pkg)
    set_path(monkeypatch, path, layout)
    s, hook, runs = build_system(pkg, scene)
    s.initialize()
    assert s.info()["dense_solve"] == (1 if path == "dense" else 0)
    assert multi_row_slots(scene, runs) >= 3, "no (node, component) slot fed by several rows of one user force"

    # (a) the local step: D_i x the hook receives and the u, z it leaves, bitwise the oracle's (three calls, carried u and warm start)
    o_ls = scene.oracle()
    for call, amp in enumerate((0.01, 0.05, 0.2)):
        xs = scene.x.ravel() * (1.0 + amp * np.sin(np.arange(scene.x.size) * (1.0 + call)))
        hook.dx.clear()
        s.local_step_only(xs)
        uo, zo = o_ls.local_step(xs, scene.dt)
        assert len(hook.dx) == 1
        Dx = dx_reference(o_ls, xs)
        for b, f0, erp, g0, orows in runs:
            assert np.array_equal(hook.dx[0][g0:g0 + erp[-1]], Dx[orows]), (name, call, b, "D_i x")
            got = s.read_local(b)
            assert np.array_equal(got["u"], uo[orows], equal_nan=True) and np.array_equal(got["z"], zo[orows], equal_nan=True), (name, call, b, "u, z")

    # (b) one ADMM iteration with residual tracking: against the oracle's step() and the built-in batches of the same scene
    s, hook, runs = build_system(pkg, scene)
    s.initialize(); s.enable_residuals(True)
    bi, _, _ = build_system(pkg, scene, restate=False)
    bi.initialize()
    o = scene.oracle(1); o.track_residuals(True)
    s.step(1); bi.step(1); o.step()
    x, xo, xb = s.m_x, o.x, bi.m_x
    assert np.abs(x - xo).max() < 1e-11, (name, "vs oracle", float(np.abs(x - xo).max()))
    assert np.abs(x - xb).max() <= 1e-12 * np.abs(xb).max(), (name, "vs built-in", float(np.abs(x - xb).max()))
    r, sd, n = s.residuals(); ro, so, no = o.residuals()
    assert n == no == 1
    close_residuals(r, sd, ro, so)

    # (c) a frame of several iterations (kinds without a truncated minimiser): |r| and |s| of every iteration
    if scene.iters > 1:
        s, hook, runs = build_system(pkg, scene)
        s.initialize(); s.enable_residuals(True)
        o = scene.oracle(scene.iters); o.track_residuals(True)
        s.step(scene.iters); o.step()
        r, sd, n = s.residuals(); ro, so, no = o.residuals()
        assert n == no == scene.iters
        close_residuals(r, sd, ro, so)
        assert np.abs(s.m_x - o.x).max() < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["dense", "panels"])
@pytest.mark.parametrize("name", ["bar", "cloth"])
def test_restated_user_forces_recompute_weights(pkg, monkeypatch, name, path):
    """set_weights on generic (and built-in) batches + recompute_weights: solves against SparseReference.with_weights at the bounds
    of test_wide_supernodes.py, then one frame against the oracle with the same edited weights (orc_recompute_weights)"""
    scene = SCENES[name](pkg)
    set_path(monkeypatch, path, "rank_major")
    s, hook, runs = build_system(pkg, scene)
    s.initialize()
    assert s.info()["dense_solve"] == (1 if path == "dense" else 0)
    o = scene.oracle(scene.iters)
    ref = SparseReference(o, scene.m3, scene.dt)
    w = o.weights() * np.random.default_rng(3).uniform(0.3, 3.0, size=o.n_forces)
    user = {f0 for _, f0, _, _, _ in runs}
    b = 0
    for (kind, idx, par, u), f0 in zip(scene.forces, scene.first_force()):
        n = np.asarray(idx).reshape(-1, checkers.KIND_NODES[KIND[kind]]).shape[0]
        s.set_weights(b, np.repeat(w[f0:f0 + n], KIND_ROWS[KIND[kind]]) if f0 in user else w[f0:f0 + n])
        b += 1
    s.recompute_weights()
    ref = ref.with_weights(w)
    for i, rhs in enumerate(checkers.solve_rhs(5, scene.x, scene.m3)):
        xr, _, _ = ref.solve(rhs)
        xs = s.solve_only(rhs)
        err = float(np.abs(xs - xr).max() / np.abs(xr).max())
        assert err <= fwd_tol(ref.kappa1), (name, i, err, ref.kappa1)
        assert ref.backward_error(xs, rhs) <= BWD_ERR_TOL, (name, i)
    o.set_weights(w)
    hook.o.set_weights(w)
    s.step(scene.iters); o.step()
    assert np.abs(s.m_x - o.x).max() < 1e-10, (name, float(np.abs(s.m_x - o.x).max()))


# ---------------------------------------------------------------- 2. irregular user rows, extended-precision reference ----
def irregular_scene(pkg):
    """a corotational bar (built-in) between two generic batches of irregular rows, anchors (built-in) after the first.
    -> (x, m3, built-in forces, [(elem_row_ptr, rows, cols, vals, row weights)] * 2, the node fed by all three)"""
    mg = pkg.meshgen
    x, t = mg.bar(4, 4, 10)
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    n = x.shape[0]
    rng = np.random.default_rng(17)
    hub = int(n // 2)                                             # fed by both generic batches and the tets
    xyz = np.arange(3)

    def rows_of(pairs, r0):
        """x, y, z rows of sum_j c_j x_{node_j}: pairs = [(node, coefficient)] -> triplets for rows r0..r0+2"""
        tr, tc, tv = [], [], []
        for comp in range(3):
            for node, c in pairs:
                tr.append(r0 + comp); tc.append(3 * node + comp); tv.append(c)
        return tr, tc, tv

    # batch A: springs with coefficients other than +-1, an element of two parts with different weights (node `hub` twice per
    # component), an empty row, an element without rows
    A_erp, A_t, A_w = [0], ([], [], []), []

    def elem(parts, weights, empty=0):
        r0 = A_erp[-1]
        for k, (pairs, wk) in enumerate(zip(parts, weights)):
            tr, tc, tv = rows_of(pairs, r0 + 3 * k)
            A_t[0].extend(tr); A_t[1].extend(tc); A_t[2].extend(tv); A_w.extend([wk] * 3)
        A_w.extend([7.0] * empty)
        A_erp.append(r0 + 3 * len(parts) + empty)
    elem([[(hub, 1.0), (hub + 1, -1.0)]], [30.0])
    elem([[(hub, 0.7), (hub - 5, -1.3)], [(hub, 2.5)]], [25.0, 4.0], empty=1)
    elem([], [])                                                  # an element with no rows
    for _ in range(40):
        i, j = rng.choice(n, 2, replace=False)
        c = float(rng.uniform(0.2, 3.0))
        elem([[(int(i), c), (int(j), -c * float(rng.uniform(0.5, 1.5)))]], [float(rng.uniform(1.0, 40.0))])
    A = (np.array(A_erp, np.int32), np.array(A_t[0], np.int32), np.array(A_t[1], np.int32), np.array(A_t[2]), np.array(A_w))

    # batch B: a centroid force over 50 nodes (coefficients 1/k, `hub` among them), elements of two edges sharing a node
    B_erp, B_t, B_w = [0], ([], [], []), []
    k = 50
    cent = np.concatenate([[hub], rng.choice(np.setdiff1d(np.arange(n), [hub]), k - 1, replace=False)])
    tr, tc, tv = rows_of([(int(v), 1.0 / k) for v in cent], 0)
    B_t[0].extend(tr); B_t[1].extend(tc); B_t[2].extend(tv); B_w.extend([12.0] * 3); B_erp.append(3)
    for _ in range(30):
        a, b, c = (int(v) for v in rng.choice(n, 3, replace=False))
        r0 = B_erp[-1]
        for q, (pairs, wk) in enumerate((([(a, 1.0), (b, -0.5)], 9.0), ([(a, -2.0), (c, 1.5)], 3.0))):
            tr, tc, tv = rows_of(pairs, r0 + 3 * q)
            B_t[0].extend(tr); B_t[1].extend(tc); B_t[2].extend(tv); B_w.extend([wk] * 3)
        B_erp.append(r0 + 6)
    p = rng.permutation(len(B_t[0]))
    B = (np.array(B_erp, np.int32), np.array(B_t[0], np.int32)[p], np.array(B_t[1], np.int32)[p], np.array(B_t[2])[p], np.array(B_w))
    builtin = [("TET_LINEAR", t, [4000.0]), ("ANCHOR", mg.bar_anchor_nodes(4, 4), [-1.0, 1.0])]
    return x, m3, builtin, [A, B], hub


class TargetHook:
    """project() of the irregular rows: every row pulled toward a fixed target, z = (Dx + u + a t) / (1 + a), u += Dx - z, for this
    rank's elements; records the u and z it returns"""

    def __init__(self, s, batches, targets, a=0.5):
        self.s, self.batches, self.t, self.a, self.last = s, batches, targets, a, None

    def __call__(self, dt, Dx, u, z):
        for b, erp, g0 in self.batches:
            for e in self.s.local_elements(b):
                r = slice(g0 + int(erp[e]), g0 + int(erp[e + 1]))
                d = Dx[r] + u[r]
                z[r] = (d + self.a * self.t[r]) / (1.0 + self.a)
                u[r] += Dx[r] - z[r]
        self.last = (u.copy(), z.copy())


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["dense", "panels"])
def test_irregular_user_rows_against_extended_precision(pkg, monkeypatch, path):
    set_path(monkeypatch, path, "rank_major")
    x, m3, builtin, gens, hub = irregular_scene(pkg)
    s = pkg.System(device_id=0); s.set_timestep(DT)
    s.add_nodes(x.ravel(), m3)
    b_tet = s.add_forces(KIND["TET_LINEAR"], *builtin[0][1:])
    b_A = s.add_generic(*gens[0])
    b_anc = s.add_forces(KIND["ANCHOR"], *builtin[1][1:])
    b_B = s.add_generic(*gens[1])
    s.add_gravity(GRAVITY)
    nA = int(gens[0][0][-1])
    rng = np.random.default_rng(4)
    targets = rng.normal(scale=0.05, size=nA + int(gens[1][0][-1]))
    hook = TargetHook(s, [(b_A, gens[0][0], 0), (b_B, gens[1][0], nA)], targets)
    s.set_project_hook(hook)
    s.initialize()
    assert s.info()["dense_solve"] == (1 if path == "dense" else 0)
    # the shapes: an empty row, an element without rows, a (node, component) slot fed by several rows of one element, the hub in all three
    erpA = gens[0][0]
    assert np.any(np.diff(erpA) == 0) and np.bincount(gens[0][1], minlength=nA).min() == 0
    o = Oracle(); o.settings(DT, 1)
    o.add_nodes(x.ravel(), m3)
    for kind, idx, par in builtin:
        o.add_forces(KIND[kind], idx, par)
    assert o.initialize()
    rr, cc, vv = o.D_triplets()
    assert np.any(cc // 3 == hub) and hub in gens[0][2] // 3 and hub in gens[1][2] // 3
    s.step(1)
    xd = s.m_x
    assert hook.last is not None
    ug, zg = hook.last
    # u, z of every batch (built-in: read_local, element after element in the oracle's row order; generic: what the hook returned)
    gi = o.global_idx(); nt = builtin[0][1].shape[0]
    lt, la = s.read_local(b_tet), s.read_local(b_anc)
    q_bi = np.zeros(o.rows)
    q_bi[gi[0]:gi[0] + 9 * nt] = (lt["z"] - lt["u"]).ravel()
    q_bi[gi[nt]:gi[nt] + la["u"].size] = (la["z"] - la["u"]).ravel()
    rA, rB = s.read_local(b_A), s.read_local(b_B)
    assert np.array_equal(rA["u"], ug[:nA]) and np.array_equal(rB["z"], zg[nA:])
    # the whole selector as explicit triplets: the oracle's rows of the built-in forces, then batch A's, then batch B's
    R = o.rows
    D = (np.concatenate([rr, gens[0][1] + R, gens[1][1] + R + nA]), np.concatenate([cc, gens[0][2], gens[1][2]]),
         np.concatenate([vv, gens[0][3], gens[1][3]]))
    W = np.concatenate([o.wdiag, gens[0][4], gens[1][4]])
    ref = SparseReference.from_selector(D, W, m3, DT)
    v = np.tile(np.array(GRAVITY) * DT, x.shape[0])              # v after the explicit gravity of the first frame
    ld = np.longdouble
    m_xbar = np.asarray(m3, dtype=ld) * (x.ravel().astype(ld) + ld(DT) * v.astype(ld))
    b_ref = ref.rhs(m_xbar, np.concatenate([q_bi, zg - ug]))
    xr, _, _ = ref.solve(b_ref)
    err = float(np.abs(xd - xr).max() / np.abs(xr).max())
    assert err <= fwd_tol(ref.kappa1), ("forward error", err, ref.kappa1)
    assert ref.backward_error(xd, b_ref) <= BWD_ERR_TOL


# ---------------------------------------------------------------- 3. elements that span ranks ----
SPAN_DIMS = (6, 6, 40)


def span_system(pkg, force, device_id, rank=0, world=1, mode=None):
    """the corotational 6x6x40 bar with one user element whose nodes lie far apart: "pin" (3 rows at each end of the bar, pulled
    toward targets) or "collision" (identity rows over every node, clamped above a floor in the hook); None: the bar alone, whose
    sparsity pattern and so whose partition are the same (either element couples each of its nodes with itself only)"""
    mg = pkg.meshgen
    x, t = mg.bar(*SPAN_DIMS)
    n = x.shape[0]
    s = pkg.System(device_id=device_id); s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3))
    s.add_forces(KIND["TET_LINEAR"], t, [4000.0])
    s.add_forces(KIND["ANCHOR"], mg.bar_anchor_nodes(*SPAN_DIMS[:2]), [-1.0, 1.0])
    b = -1
    if force == "pin":
        nodes = np.array([0, n - 1])
        rows = np.arange(6, dtype=np.int32)
        cols = (3 * np.repeat(nodes, 3) + np.tile(np.arange(3), 2)).astype(np.int32)
        b = s.add_generic([0, 6], rows, cols, np.ones(6), np.full(6, 20.0))
        target = x[nodes].ravel() + np.array([0.0, 0.05, 0.0, 0.02, 0.1, -0.03])

        def project(dt, Dx, u, z):
            if s.local_elements(b).size:
                d = Dx + u
                z[:] = (d + 0.5 * target) / 1.5
                u += Dx - z
    elif force == "collision":
        rows = np.arange(3 * n, dtype=np.int32)
        b = s.add_generic([0, 3 * n], rows, rows, np.ones(3 * n), np.full(3 * n, 32.0))
        floor = float(x[:, 1].min()) - 0.004

        def project(dt, Dx, u, z):       # CollisionForce::project with a floor shape
            if s.local_elements(b).size:
                d = Dx + u
                zz = d.copy()
                y = zz[1::3]
                np.maximum(y, floor, out=y)
                z[:] = zz
                u += Dx - z
    if b >= 0:
        s.set_project_hook(project)
    s.add_gravity(GRAVITY)
    if world > 1:
        s.set_shard(rank, world)
        s.set_shard_mode(mode)
    s.user_batch = b
    return s


def span_env(monkeypatch, dist_top):
    """host-only contexts planned like device ones (rank-local factorization, the distributed top), the panel path"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_PLAN_AS_IF_DEVICE", "1")
    monkeypatch.setenv("ADMM_HIP_DIST_TOP", "1" if dist_top else "0")


def user_nodes(force):
    n = np.prod(np.array(SPAN_DIMS) + 1)
    return np.array([0, n - 1]) if force == "pin" else np.arange(n)


@pytest.mark.parametrize("dist_top", [False, True])
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("force", ["pin", "collision"])
def test_subtree_sharding_refuses_an_element_across_ranks(pkg, monkeypatch, force, world, dist_top):
    """host-only contexts (planned as if on a device): the user element's nodes lie in two ranks' subtrees (shown by the same scene
    without it, whose partition is the same: the element adds no coupling between them); every rank's initialize() refuses with
    ADMM_ERR_UNSUPPORTED, naming the batch, the element and two ranks; contiguous sharding accepts the scene."""
    span_env(monkeypatch, dist_top)
    plain = []
    for r in range(world):      # the same bar without the user element
        s = span_system(pkg, None, -1, r, world, "subtree")
        s.initialize()
        plain.append(s)
    owner = plain[0].node_owner()
    assert plain[0].info()["dist_top"] == (1 if dist_top else 0)
    used = owner[user_nodes(force)]
    assert np.unique(used[used >= 0]).size >= 2, "the user element's nodes do not span two ranks' subtrees"
    for r in range(world):
        s = span_system(pkg, force, -1, r, world, "subtree")
        with pytest.raises(pkg.AdmmHipError, match=r"element 0 of generic batch 2 has node \d+ in rank \d+'s subtree and node \d+ in rank \d+'s.*ADMM_SHARD_CONTIGUOUS") as ei:
            s.initialize()
        assert "error 4:" in str(ei.value)                        # ADMM_ERR_UNSUPPORTED
    for r in range(world):
        s = span_system(pkg, force, -1, r, world, "contiguous")
        s.initialize()


def run_ranks(shards, frames, iters):
    world = len(shards)
    out, errs = [None] * world, []

    def run(r):
        try:
            xs = []
            for _ in range(frames):
                shards[r].step(iters)
                xs.append(shards[r].m_x.copy())
            out[r] = (xs, shards[r].m_v.copy())
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    return out


def thread_allreduce_hooks(world):
    from test_sharding import _thread_allreduce_hooks
    return _thread_allreduce_hooks(world)


@pytest.mark.gpu
@pytest.mark.parametrize("force", ["pin", "collision"])
def test_user_element_across_ranks(pkg, monkeypatch, force):
    """N contexts on one GPU (one host thread per rank, meeting in the all-reduce hook), panel sweeps.  Subtree sharding at 2 and 3
    ranks (replicated top) and at 2 (distributed top): the element's nodes lie in two ranks' subtrees and every rank refuses it at
    initialize.  Contiguous sharding at 2 and 3 ranks: three frames within 1e-9 of the one-rank run, all ranks bitwise equal."""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    ref = span_system(pkg, force, 0)
    ref.initialize()
    assert ref.info()["dense_solve"] == 0
    refx = []
    for _ in range(3):
        ref.step(10); refx.append(ref.m_x.copy())
    assert np.abs(refx[-1] - refx[0]).max() > 1e-3              # the scene moves
    for world, dist in ((2, "0"), (3, "0"), (2, "1")):
        monkeypatch.setenv("ADMM_HIP_DIST_TOP", dist)
        plain = [span_system(pkg, None, 0, r, world, "subtree") for r in range(world)]
        hooks = thread_allreduce_hooks(world)
        for r, s in enumerate(plain):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(plain)
        owner = plain[0].node_owner()
        assert plain[0].info()["dist_top"] == int(dist)
        used = owner[user_nodes(force)]
        assert np.unique(used[used >= 0]).size >= 2, (world, dist, "the user element's nodes do not span two ranks' subtrees")
        del plain
        shards = [span_system(pkg, force, 0, r, world, "subtree") for r in range(world)]
        hooks = thread_allreduce_hooks(world)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        with pytest.raises(pkg.RankErrors) as ei:
            pkg.initialize_together(shards)
        for e in ei.value.errors:
            assert isinstance(e, pkg.AdmmHipError) and "ADMM_SHARD_CONTIGUOUS" in str(e) and "still inside" not in str(e), (world, dist, e)
        del shards
    monkeypatch.delenv("ADMM_HIP_DIST_TOP")
    for world in (2, 3):
        shards = [span_system(pkg, force, 0, r, world, "contiguous") for r in range(world)]
        hooks = thread_allreduce_hooks(world)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(shards)
        assert sum(s.local_elements(s.user_batch).size for s in shards) == 1
        out = run_ranks(shards, 3, 10)
        for r in range(world):
            xs, vs = out[r]
            for f in range(3):
                assert np.abs(xs[f] - refx[f]).max() < 1e-9, (world, r, f, float(np.abs(xs[f] - refx[f]).max()))
            assert np.array_equal(xs[-1], out[0][0][-1]) and np.array_equal(vs, out[0][1])


# ---------------------------------------------------------------- CPU: the scenes' assembly ----
@pytest.mark.parametrize("name", ["bar", "cloth", "delaunay"])
def test_restated_forces_assemble_the_builtin_system(pkg, name):
    """host-only contexts: the restated scene (shuffled triplets, split duplicates) passes the K (x) I3 check and assembles the
    built-in scene's A to rounding; every (node, component) slot of a tet / hinge is fed by several rows of one user force"""
    scene = SCENES[name](pkg)
    s, _, runs = build_system(pkg, scene, device_id=-1)
    s.initialize()
    b, _, _ = build_system(pkg, scene, restate=False, device_id=-1)
    b.initialize()
    assert multi_row_slots(scene, runs) >= 3
    v = np.random.default_rng(1).normal(size=scene.x.size)
    ya, yb = s.apply_A(v), b.apply_A(v)
    assert np.abs(ya - yb).max() <= 1e-14 * np.abs(yb).max()


def test_irregular_rows_assemble_the_selector_reference(pkg):
    """host-only context of the irregular scene: A = M + dt^2 D^T W^2 D of SparseReference.from_selector over the same explicit triplets"""
    x, m3, builtin, gens, hub = irregular_scene(pkg)
    s = pkg.System(device_id=-1); s.set_timestep(DT)
    s.add_nodes(x.ravel(), m3)
    s.add_forces(KIND["TET_LINEAR"], *builtin[0][1:])
    s.add_generic(*gens[0])
    s.add_forces(KIND["ANCHOR"], *builtin[1][1:])
    s.add_generic(*gens[1])
    s.initialize()
    o = Oracle(); o.settings(DT, 1)
    o.add_nodes(x.ravel(), m3)
    for kind, idx, par in builtin:
        o.add_forces(KIND[kind], idx, par)
    assert o.initialize()
    rr, cc, vv = o.D_triplets()
    R, nA = o.rows, int(gens[0][0][-1])
    ref = SparseReference.from_selector((np.concatenate([rr, gens[0][1] + R, gens[1][1] + R + nA]), np.concatenate([cc, gens[0][2], gens[1][2]]),
                                         np.concatenate([vv, gens[0][3], gens[1][3]])), np.concatenate([o.wdiag, gens[0][4], gens[1][4]]), m3, DT)
    v = np.random.default_rng(2).normal(size=x.size)
    y = ref.A @ v
    assert np.abs(s.apply_A(v) - y).max() <= 1e-14 * np.abs(y).max()
    b = ref.rhs(m3 * x.ravel(), ref.D @ x.ravel())                 # z - u = D x: b = A x
    xr, _, _ = ref.solve(b)
    assert np.abs(xr - x.ravel()).max() <= 1e-12 * np.abs(x).max()
