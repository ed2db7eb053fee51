"""Per-iteration ADMM residuals (admm_hip_enable_residuals / admm_hip_set_tolerance) against an extended-precision reference.

No trajectories are compared (the truncated L-BFGS makes the library's and the oracle's diverge inside a frame).  Instead the DEVICE's own
states on both sides of iteration j are read out and r_j, s_j recomputed from them in np.longdouble (checkers.ResidualReference, D and W from the
oracle).  Frames are bitwise reproducible, the end of admm_hip_step leaves u and z alone, and with tracking on z is always stored: from identical
starts (optionally after whole frames) a system that runs step(j) holds x_j = m_x, u_j, z_j, and a twin that runs step(j + 1) holds u_{j+1},
z_{j+1}; a third system with tracking on reports r[0..k), s[0..k).

Tolerances are derived, not measured (ResidualReference's docstring): |r_dev - r_ref| <= c_r EPS r_ref with c_r from the kernels' summation
depth, the D x form with the roundings of u + (Dx - z) and of D x on top, |s_dev - s_ref| <= gamma_m ||D^T| W^2 |dz|| + c_s EPS s_ref.  Every case
also asserts, with CPU arithmetic only, that removing the LAST element of each batch (the tail of the last partial block) moves both reference
values by at least 1000 tolerances: a dropped tail, a stale slot or a wrong w^2 on one element cannot hide below the bound.

Where the sensitivity condition is asserted.  The comparison with the derived bounds runs at EVERY checked iteration (0..3 of frame 1 and of frame 3)
in all three forms.  The sensitivity of an element's share is a property of the physics at that iteration and cannot hold everywhere: a static
anchor's z is its target, so its share of s is identically zero after a frame's first iteration (asserted to be exactly zero); at a frame's first
iteration the bound on s carries the rounding of the device's warm start D m_x, gamma ||D^T| W^2 |D||m_x||, which is of the size of one element's
share; an element inside its limits or outside every shape has z = Dx + u and no share of r; late in a long frame r has fallen below the absolute
roundings of D x that the Dx form's bound contains.  So every case prints the whole table and asserts, for EVERY batch and EACH of the three
quantities, that the last element is worth at least 1000 tolerances at one or more of the case's checked iterations (assert_sensitivity); the scenes'
starts and limits are chosen so that this holds.

The CPU test runs the same reconstruction on the oracle's own states and reproduces the oracle's track_residuals output to 1e-12.
"""
import threading

import numpy as np
import pytest

from checkers import KIND, KIND_NODES, Oracle, ResidualReference, deformed_start
from test_sharding import _thread_allreduce_hooks

# the reference needs an extended long double (x86: 2^-63); decided before any work
pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps > 2.0 ** -63, reason="np.longdouble has no extended precision on this host")
gpu = pytest.mark.gpu
DT = 0.04
GRAVITY = (0.0, -9.8, 0.0)


def _mg():
    from __graft_entry__ import load_package
    return load_package().meshgen


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes: dict(x [n][3], m3 [3n], forces [(kind, idx, params)], start [3n] or None, shapes (types, params) or None, lib_setup or None)
# ---------------------------------------------------------------------------------------------------------------------------------
# (TET_VOLUME and TRI_AREA with limits ABOVE 1: the rest state itself is outside them, every element projects in every iteration)
TET_PARAMS = dict(TET_LINEAR=[4000.0], TET_VOLUME=[4000.0, 1.05, 1.10], TET_NH=[1e5, 1e5, 5], TET_STVK=[1e5, 1e5, 5])


def bar_scene(kind="TET_NH", dims=(3, 3, 7), n_tets=None, anchors=True):
    """a bar of one tet kind, anchored on its k = 0 face, started from checkers.deformed_start (the anchors keep their rest targets and pull)"""
    mg = _mg()
    x, t = mg.bar(*dims)
    if n_tets is not None:
        t = t[:n_tets]
        assert np.unique(t).size == x.shape[0]
    m3 = np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3)
    forces = [(kind, t, TET_PARAMS[kind])]
    if anchors:
        forces.append(("ANCHOR", mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0]))
    return dict(x=x, m3=m3, forces=forces, start=deformed_start(x))


def _wrinkle(x):
    """a smooth deformation of a sheet in the xz-plane from + and * only: in-plane stretch and out-of-plane bending"""
    q = x.copy()
    q[:, 0] = x[:, 0] + 0.10 * (x[:, 2] * x[:, 2]) + 0.04 * (x[:, 0] * x[:, 2])
    q[:, 1] = x[:, 1] + 0.12 * (x[:, 0] * x[:, 2]) - 0.08 * (x[:, 2] * x[:, 2]) + 0.06 * (x[:, 0] * x[:, 0])
    q[:, 2] = x[:, 2] + 0.06 * (x[:, 0] * x[:, 0])
    return q


SHEET_PARAMS = dict(TRI_STRAIN=[100.0, 0.95, 1.05, 1.0], TRI_AREA=[100.0, 4, 1.15, 1.30], TRI_FUNG=[50.0, 0.5, 2.0], BEND=[20.0], SPRING=[50.0])


def sheet_scene(kind="TRI_STRAIN", w=5, l=7, size=1.0, floor=None, banded=False):
    """a sym-plane sheet of ONE kind (triangles, hinges or springs along the triangle edges) hanging from two corner anchors; floor: a
    collision batch over all nodes against a floor at that height, placed so that the wrinkled start puts nodes (the last one too) below it"""
    mg = _mg()
    x, tris = mg.sym_plane(w, l, size=size)
    n = x.shape[0]
    if banded:      # nodes renumbered along the strip: the oracle factors in natural order, the cell centres would otherwise couple far-apart numbers
        long_axis = 2 if np.ptp(x[:, 2]) >= np.ptp(x[:, 0]) else 0
        order = np.lexsort((x[:, 2 - long_axis], x[:, long_axis]))
        inv = np.empty(n, np.int64); inv[order] = np.arange(n)
        x = x[order]; tris = inv[tris].astype(np.int32)
    if kind == "BEND":
        idx = mg.bend_hinges(tris)
    elif kind == "SPRING":
        e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
        idx = np.unique(e, axis=0).astype(np.int32)
    else:
        idx = tris
    forces = [(kind, idx, SHEET_PARAMS[kind]), ("ANCHOR", (np.array([0, 1], np.int32) if banded else np.array([0, w], np.int32)), [-1.0, 1.0])]
    sc = dict(x=x, m3=np.full(3 * n, 0.5 / n), forces=forces, start=_wrinkle(x).ravel())
    if floor is not None:
        forces.append(("COLLISION", np.arange(n, dtype=np.int32), [32.0]))
        y = sc["start"].reshape(-1, 3)[:, 1]
        h = float(max(np.median(y), y[-1] + 0.01)) if floor == "auto" else float(floor)
        sc["shapes"] = ([0, 1], [[0.0, h, 0.0, 0.0], [0.3, h, 0.4, 0.25]])      # a floor and a sphere resting in it
    return sc


def collision_scene(n_side=9):
    """free nodes on a grid around a floor with a sphere on it: a collision batch alone (D = I), about half the nodes penetrating"""
    g = np.arange(n_side, dtype=np.float64) * 0.1
    X, Z = np.meshgrid(g, g, indexing="ij")
    x = np.stack([X.ravel(), 0.0 * X.ravel(), Z.ravel()], axis=1)
    n = x.shape[0]
    start = x.copy()
    start[:, 1] = 0.04 * (x[:, 0] * x[:, 2]) - 0.02 * x[:, 0] - 0.015      # below the floor y = 0 where x z is small; the last node too
    start[-1, 1] = -0.03
    return dict(x=x, m3=np.full(3 * n, 0.01), forces=[("COLLISION", np.arange(n, dtype=np.int32), [32.0])], start=start.ravel(),
                shapes=([0, 1], [[0.0, 0.0, 0.0, 0.0], [0.43, 0.0, 0.37, 0.15]]))      # (centre off the grid: no node is pushed onto it)


def mixed_scene(mesh=False):
    """tets (NH lower half, StVK upper half) + triangles + hinges + springs + anchors + a collision batch over all nodes, one shared slot array.
    mesh: the collision batch also meets a registered closed mesh (a small box under the bar's free end) and the bar's own surface"""
    mg = _mg()
    dims = (3, 3, 9)
    x, t = mg.bar(*dims)
    m = mg.lumped_tet_mass(x, t, 1000.0)
    half = t.shape[0] // 2
    xc, tris = mg.sym_plane(5, 6, size=0.5)
    xc = xc + np.array([0.4, 0.1, 0.0])
    off = x.shape[0]
    X = np.concatenate([x, xc]); n = X.shape[0]
    M = np.concatenate([m, np.full(xc.shape[0], 0.5 / xc.shape[0])])
    e = np.unique(np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1), axis=0).astype(np.int32)
    start = X.copy(); start[:off] = deformed_start(x).reshape(-1, 3); start[off:] = _wrinkle(xc - np.array([0.4, 0.1, 0.0])) + np.array([0.4, 0.1, 0.0])
    floor_y = float(start[-1, 1] + 0.01)
    forces = [("TET_NH", t[:half], TET_PARAMS["TET_NH"]), ("TET_STVK", t[half:], TET_PARAMS["TET_STVK"]),
              ("TRI_STRAIN", tris + off, SHEET_PARAMS["TRI_STRAIN"]), ("BEND", mg.bend_hinges(tris) + off, SHEET_PARAMS["BEND"]),
              ("SPRING", e[::2] + off, SHEET_PARAMS["SPRING"]),
              ("ANCHOR", np.concatenate([mg.bar_anchor_nodes(dims[0], dims[1]), np.array([off, off + 5], np.int32)]), [-1.0, 1.0]),
              ("COLLISION", np.arange(n, dtype=np.int32), [32.0])]
    sc = dict(x=X, m3=np.repeat(M, 3), forces=forces, start=start.ravel(), shapes=([0], [[0.0, floor_y, 0.0, 0.0]]))
    if mesh:
        xb, tb = mg.bar(1, 1, 1, 0.08)
        box = xb + np.array([0.02, -0.07, 0.36]); box_tris = mg.tet_surface(tb, xb)
        used = np.unique(box_tris); box_v = box[used]; box_t = np.searchsorted(used, box_tris).astype(np.int32)
        surf = mg.tet_surface(t, x)

        def lib_setup(s):
            mid = s.add_collision_mesh(box_v, box_t)
            ib = s.add_body_surface(0, off, surf)
            s.set_collision_shapes([0, 3, 3], [[0.0, floor_y, 0.0, 0.0], [0.0, 0.0, 0.0, mid], [0.0, 0.0, 0.0, ib]])
        sc["lib_setup"] = lib_setup
    return sc


# ---------------------------------------------------------------------------------------------------------------------------------
# the two sources of states: the oracle (CPU) and the library (GPU, one or more ranks)
# ---------------------------------------------------------------------------------------------------------------------------------
def make_oracle(sc, iters=1):
    o = Oracle(); o.settings(DT, iters)
    o.add_nodes(sc["x"].ravel(), sc["m3"])
    for kind, idx, par in sc["forces"]:
        o.add_forces(KIND[kind], idx, par)
    o.add_gravity(GRAVITY)
    if sc.get("shapes"):
        o.set_collision_shapes(*sc["shapes"])
    assert o.initialize()
    if sc.get("start") is not None:
        o.x = sc["start"]
    return o


def batch_sizes(sc):
    return [np.asarray(f[1]).reshape(-1, KIND_NODES[KIND[f[0]]]).shape[0] for f in sc["forces"]]


def batch_first(sc):
    """the oracle's force index of every batch's element 0 (and the total)"""
    return np.concatenate([[0], np.cumsum(batch_sizes(sc))])


class OracleSim:
    def __init__(self, sc, track=False):
        self.o = make_oracle(sc); self.o.track_residuals(track)

    def step(self, k):
        self.o.settings(DT, k); self.o.step()

    def state(self):
        return dict(x=self.o.x, u=self.o.u, z=self.o.z)

    def residuals(self):
        r, s, n = self.o.residuals()
        return [(r, s, n)]


class LibSim:
    """the library's System of a scene on `world` ranks (one GPU); state() in the oracle's row order through ref"""

    def __init__(self, pkg, sc, ref, track=False, world=1, mode=None, tolerance=None):
        self.ref, self.sc, self.world = ref, sc, world
        self.sys = []
        for r in range(world):
            s = pkg.System(device_id=0); s.set_timestep(DT)
            s.add_nodes(sc["x"].ravel(), sc["m3"])
            for kind, idx, par in sc["forces"]:
                s.add_forces(pkg.KIND[kind], idx, par)
            s.add_gravity(GRAVITY)
            if sc.get("lib_setup"):
                sc["lib_setup"](s)
            elif sc.get("shapes"):
                s.set_collision_shapes(*sc["shapes"])
            if world > 1:
                s.set_shard(r, world); s.set_shard_mode(mode)
            self.sys.append(s)
        if world > 1:
            for s, h in zip(self.sys, _thread_allreduce_hooks(world)):
                s.set_allreduce(h)
            pkg.initialize_together(self.sys)
        else:
            self.sys[0].initialize()
        for s in self.sys:
            if sc.get("start") is not None:
                s.m_x = sc["start"]
            if tolerance:
                s.set_tolerance(*tolerance)
            elif track:
                s.enable_residuals(True)
        self.first = batch_first(sc)
        # the device's weights and row layout are bitwise the oracle's (everything else in the reference is the oracle's alone)
        for b, (kind, idx, par) in enumerate(sc["forces"]):
            rest = self.sys[0].read_rest(b)
            f0, f1 = self.first[b], self.first[b + 1]
            assert np.array_equal(rest["weight"], ref.weights[f0:f1]) and np.array_equal(rest["global_idx"], ref.gidx[f0:f1]), kind

    def _all(self, fn):
        if self.world == 1:
            return [fn(self.sys[0])]
        out = [None] * self.world; errs = []

        def run(r):
            try:
                out[r] = fn(self.sys[r])
            except Exception as e:  # noqa: BLE001
                errs.append((r, repr(e)))
        th = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        [t.start() for t in th]; [t.join(timeout=300) for t in th]
        assert not errs and all(t is not None and not t.is_alive() for t in th), errs
        return out

    def step(self, k):
        self._all(lambda s: s.step(k))

    def state(self):
        u = np.full(self.ref.rows, np.nan); z = np.full(self.ref.rows, np.nan); seen = np.zeros(self.ref.rows, np.int32)
        for s in self.sys:
            for b, (kind, idx, par) in enumerate(self.sc["forces"]):
                ids = s.local_elements(b)
                if ids.size == 0:
                    continue
                d = s.read_local(b)
                rows = self.ref.rows_of(self.first[b], ids, KIND[kind])
                u[rows] = d["u"]; z[rows] = d["z"]; seen[rows] += 1
        assert (seen == 1).all()      # the ranks' elements partition every batch
        xs = [s.m_x for s in self.sys]
        assert all(np.array_equal(xs[0], x) for x in xs)
        return dict(x=xs[0], u=u, z=z)

    def full(self):
        """everything a frame leaves behind, for bitwise comparisons: m_x, m_v and per batch u and the warm-start state"""
        s = self.sys[0]
        out = [s.m_x, s.m_v]
        for b in range(len(self.sc["forces"])):
            d = s.read_local(b)
            out += [d["u"], d["state"]]
        return out

    def residuals(self):
        return [s.residuals() for s in self.sys]


# ---------------------------------------------------------------------------------------------------------------------------------
# the check itself
# ---------------------------------------------------------------------------------------------------------------------------------
def last_element_masks(ref, sc):
    first = batch_first(sc)
    masks = []
    for b in range(len(sc["forces"])):
        m = np.zeros(ref.rows, bool); m[ref.force_rows(first[b + 1] - 1)] = True
        masks.append(m)
    return masks


def reference_values(ref, sc, make_sim, history, iterations, per_block=64, ranks=1):
    """history: the iteration counts of the whole frames run first; iterations: the j to check in the next frame.  Twins: one fresh system
    per needed state, all from the scene's start.  -> {j: dict(r_u, r_dx, s, tol_r_u, tol_r_dx, tol_s, c_r, c_s, sens)}; sens[b] = by how many
    tolerances (r u form, r Dx form, s) the reference moves without the last element of batch b"""
    need = sorted(set(iterations) | set(j + 1 for j in iterations))
    states = {}
    x_start = None
    for k in need:
        sim = make_sim()
        for h in history:
            sim.step(h)
        if x_start is None:
            x_start = sim.state()["x"]
        sim.step(k)
        states[k] = sim.state()
    # partials per batch: one per `per_block` tets / 64 anchors where the projection kernel tracks, one per 256 elements from the separate passes
    fused = ("TET_LINEAR", "TET_VOLUME", "TET_NH", "TET_STVK", "ANCHOR")
    ser = ref.serial(max(-(-n // ((per_block if f[0] != "ANCHOR" else 64) if f[0] in fused else 256)) for f, n in zip(sc["forces"], batch_sizes(sc))))
    c_r, c_s = ref.c_r(batches=len(sc["forces"]), serial=ser, ranks=ranks), ref.c_s(serial=ser)
    masks = last_element_masks(ref, sc)
    out = {}
    for j in iterations:
        a, b = states[j], states[j + 1]
        zprev = ref.zprev_frame_start(x_start) if j == 0 else a["z"]
        v = dict(r_u=ref.r_from_u(a["u"], b["u"]), r_dx=ref.r_from_dx(a["x"], b["z"]), s=ref.s(b["z"], zprev), c_r=c_r, c_s=c_s, serial=ser)
        v["tol_r_u"] = ref.bound_r_u(a["u"], b["u"], c_r)
        v["tol_r_dx"] = ref.bound_r_dx(a["x"], a["u"], b["u"], c_r)
        v["tol_s"] = ref.bound_s(b["z"], zprev, c_s, x_start=x_start if j == 0 else None, ranks=ranks)
        # the kernels' claim r = W (Dx - z) = W (u_new - u_old), on the device's own numbers
        assert abs(v["r_u"] - v["r_dx"]) <= v["tol_r_dx"], (j, float(v["r_u"]), float(v["r_dx"]))
        sens = []
        for bi, m in enumerate(masks):
            dr_u = abs(ref.r_from_u(a["u"], b["u"], drop=m) - v["r_u"]); dr_dx = abs(ref.r_from_dx(a["x"], b["z"], drop=m) - v["r_dx"])
            ds = abs(ref.s(b["z"], zprev, drop=m) - v["s"])
            if sc["forces"][bi][0] == "ANCHOR" and j > 0:      # a static anchor's z is its target: no share of s after the first iteration
                assert ds == 0
            sens.append((float(dr_u) / v["tol_r_u"], float(dr_dx) / v["tol_r_dx"], float(ds) / v["tol_s"]))
        v["sens"] = sens
        out[j] = v
    return out


def assert_sensitivity(name, sc, checked):
    """checked: [(label, values of reference_values at one iteration)].  For every batch and each quantity the last element must be worth >= 1000
    tolerances at one or more of the checked iterations (see the file's docstring); prints where it holds."""
    for bi, (kind, idx, par) in enumerate(sc["forces"]):
        for q, what in enumerate(("r (u form)", "r (Dx form)", "s")):
            best = max(v["sens"][bi][q] for _, v in checked)
            holds = [lab for lab, v in checked if v["sens"][bi][q] >= 1000]
            print("%-34s sensitivity %-11s batch %d %-10s holds at %d of %d: %s (best %.1e)" % (name, what, bi, kind, len(holds), len(checked), " ".join(holds), best))
            assert holds, ("the last element of the batch never moves the reference by 1000 tolerances", name, kind, what, best)


def check_frames(name, ref, sc, make_sim, make_tracked, plan, per_block=64, ranks=1, rtol=None):
    """plan: [(history of whole frames, k of the checked frame, the iterations j < k to check)].  The tracked system runs history + step(k) with
    tracking on all the way.  rtol: compare with a relative tolerance instead of the derived bounds (the CPU test against the oracle's doubles)."""
    worst = [0.0, 0.0, 0.0]
    checked = []
    for history, k, iterations in plan:
        vals = reference_values(ref, sc, make_sim, history, iterations, per_block, ranks)
        tr = make_tracked()
        for h in history:
            tr.step(h)
        tr.step(k)
        res = tr.residuals()
        for r_dev, s_dev, n in res:
            assert n == k and r_dev.size == k
            assert np.array_equal(r_dev, res[0][0]) and np.array_equal(s_dev, res[0][1])      # every rank reports the same bits
        r_dev, s_dev, _ = res[0]
        for j in iterations:
            v = vals[j]
            checked.append(("f%d.j%d" % (len(history) + 1, j), v))
            e = [abs(np.longdouble(r_dev[j]) - v["r_u"]), abs(np.longdouble(r_dev[j]) - v["r_dx"]), abs(np.longdouble(s_dev[j]) - v["s"])]
            t = [v["tol_r_u"], v["tol_r_dx"], v["tol_s"]] if rtol is None else [rtol * float(v["r_u"]), rtol * float(v["r_dx"]), rtol * float(v["s"])]
            frac = [float(e[i]) / t[i] for i in range(3)]
            print("%-34s frame %d j %3d  r %.6e s %.6e  c_r %d c_s %d serial %d  err/bound: r(u) %.3f  r(Dx) %.3f  s %.3f" %
                  (name, len(history) + 1, j, r_dev[j], s_dev[j], v["c_r"], v["c_s"], v["serial"], frac[0], frac[1], frac[2]))
            worst = [max(worst[i], frac[i]) for i in range(3)]
    print("%-34s WORST err/bound: r(u) %.3f  r(Dx) %.3f  s %.3f" % (name, worst[0], worst[1], worst[2]))
    assert worst[0] <= 1.0, ("|r_dev - r_from_u| exceeds its bound", name, worst)
    assert worst[1] <= 1.0, ("|r_dev - r_from_dx| exceeds its bound", name, worst)
    assert worst[2] <= 1.0, ("|s_dev - s_ref| exceeds its bound", name, worst)
    assert_sensitivity(name, sc, checked)


FRAMES = [([], 4, [0, 1, 2, 3]), ([5, 5], 4, [0, 1, 2, 3])]      # iterations 0..3 of frame 1 and of frame 3 (carried u and warm start)


def not_block_multiple(sc):
    for kind, idx, par in sc["forces"]:
        n = np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]]).shape[0]
        assert n % 64 != 0 and n % 256 != 0, (kind, n)


# ---- CPU: the reference and the twin-run reconstruction against the oracle's own track_residuals --------------------------------
CPU_SCENES = dict(cloth=lambda: sheet_scene("TRI_STRAIN", 5, 7), stvk_bar=lambda: bar_scene("TET_STVK", (2, 2, 5)),
                  spring_net_floor=lambda: sheet_scene("SPRING", 5, 6, floor="auto"))


@pytest.mark.parametrize("scene", sorted(CPU_SCENES))
def test_reference_reproduces_the_oracle(scene):
    """the oracle's states around each iteration (admm_iters = j and j + 1, as the twins do) -> the oracle's own |r|, |s| (plain double sums)
    to 1e-12 relative, in frame 1 and in frame 3; the sensitivity condition holds on these scenes"""
    sc = CPU_SCENES[scene]()
    ref = ResidualReference(make_oracle(sc))
    check_frames(scene, ref, sc, lambda: OracleSim(sc), lambda: OracleSim(sc, track=True), FRAMES, rtol=1e-12)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def gpu_case(pkg, name, sc, plan=FRAMES, per_block=64, world=1, mode=None):
    ref = ResidualReference(make_oracle(sc))
    check_frames(name, ref, sc, lambda: LibSim(pkg, sc, ref, world=world, mode=mode), lambda: LibSim(pkg, sc, ref, track=True, world=world, mode=mode),
                 plan, per_block=per_block, ranks=world)


KIND_SCENES = dict(
    TET_LINEAR=lambda: bar_scene("TET_LINEAR"), TET_VOLUME=lambda: bar_scene("TET_VOLUME"), TET_NH=lambda: bar_scene("TET_NH"), TET_STVK=lambda: bar_scene("TET_STVK"),
    TRI_STRAIN=lambda: sheet_scene("TRI_STRAIN"),      # (also: ANCHOR behind a non-tet batch, in its own launch)
    TRI_AREA=lambda: sheet_scene("TRI_AREA"), TRI_FUNG=lambda: sheet_scene("TRI_FUNG"), BEND=lambda: sheet_scene("BEND"), SPRING=lambda: sheet_scene("SPRING"),
    COLLISION=collision_scene)


@gpu
@pytest.mark.parametrize("kind", sorted(KIND_SCENES))
def test_every_kind_on_its_own(pkg, monkeypatch, kind):
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    sc = KIND_SCENES[kind]()
    not_block_multiple(sc)
    gpu_case(pkg, kind, sc)


VARIANTS = [("defaults", {}, 64), ("PRERED=0", {"ADMM_HIP_PRERED": "0"}, 64), ("FUSE_ANCHORS=0", {"ADMM_HIP_FUSE_ANCHORS": "0"}, 64),
            ("RES_UNFUSED=1,PRERED=0", {"ADMM_HIP_RES_UNFUSED": "1", "ADMM_HIP_PRERED": "0"}, 64),
            ("TPB=32", {"ADMM_HIP_TPB": "32"}, 32), ("TPB=16", {"ADMM_HIP_TPB": "16"}, 16), ("TPB=8", {"ADMM_HIP_TPB": "8"}, 8),
            ("SLOTS_NODE_SORTED=0", {"ADMM_HIP_SLOTS_NODE_SORTED": "0"}, 64), ("SLOTS_NODE_SORTED=1", {"ADMM_HIP_SLOTS_NODE_SORTED": "1"}, 64),
            ("dense", {"ADMM_HIP_DENSE_MAX": "2048"}, 64)]


@gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("kind", ["TET_NH", "TET_STVK"])
def test_launch_variants(pkg, monkeypatch, kind, variant):
    """an NH and a StVK bar with anchors through every slot layout and launch shape the residuals are produced in"""
    name, env, per_block = variant
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = bar_scene(kind, (3, 4, 7))
    not_block_multiple(sc)
    gpu_case(pkg, "%s %s" % (kind, name), sc, per_block=per_block)


@gpu
@pytest.mark.parametrize("kind", ["TET_NH", "TET_STVK"])
def test_cost_ordered_launch(pkg, monkeypatch, kind):
    """ADMM_HIP_TET_ORDER_MIN=8: from frame 2 on the tet blocks start in the order of their cost in the frame before; every block still
    leaves its own partial and slots"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_TET_ORDER_MIN", "8")
    sc = bar_scene(kind, (4, 4, 9))      # 864 tets = 13.5 blocks
    not_block_multiple(sc)
    assert -(-sc["forces"][0][1].shape[0] // 64) > 8      # more blocks than ADMM_HIP_TET_ORDER_MIN: the batch is launched by cost (the order itself is not readable through the ABI)
    gpu_case(pkg, "%s cost order" % kind, sc)


@gpu
@pytest.mark.parametrize("multi", ["0", "1"])
@pytest.mark.parametrize("mesh", [False, True], ids=["analytic", "mesh"])
def test_mixed_scene(pkg, monkeypatch, mesh, multi):
    """seven batches accumulate into the same |r|^2 (the accumulate flag of every batch after the first) and share the slot array of s; with a
    registered mesh and a body surface the collision batch runs in project_collision_mesh_kernel.  ADMM_HIP_LOCAL_MULTI both ways (the untracked
    twins take the one-launch local step or not)"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LOCAL_MULTI", multi)
    gpu_case(pkg, "mixed %s LOCAL_MULTI=%s" % ("mesh" if mesh else "analytic", multi), mixed_scene(mesh))


@gpu
def test_more_than_256_tet_blocks(pkg):
    """16 416 tets = 256.5 blocks of 64: sum_partials_kernel's strided serial part runs over the tet kernel's partials"""
    sc = bar_scene("TET_NH", (4, 4, 171))
    assert sc["forces"][0][1].shape[0] >= 16385 and -(-sc["forces"][0][1].shape[0] // 64) > 256
    not_block_multiple(sc)
    gpu_case(pkg, "16416 tets", sc)


@gpu
def test_more_than_65536_elements_and_dofs(pkg):
    """a strip of 65 568 triangles on 34 842 nodes: the separate passes leave more than 256 partials (257), and the gather of s has more than 256
    blocks (3n = 104 526 > 65 536): both strided sums of sum_partials_kernel"""
    sc = sheet_scene("TRI_STRAIN", 8, 2049, size=1.0, banded=True)
    assert sc["forces"][0][1].shape[0] > 65536 and 3 * sc["x"].shape[0] > 65536
    not_block_multiple(sc)
    gpu_case(pkg, "65568 triangles", sc)


@gpu
def test_growing_iteration_counts_in_one_context(pkg, monkeypatch):
    """step(3), step(70), step(130) in ONE tracked context: the result buffer grows past its first capacity twice; iterations 0, 1 and the last
    of each call"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    sc = bar_scene("TET_STVK", (2, 2, 3))
    ref = ResidualReference(make_oracle(sc))
    tr = LibSim(pkg, sc, ref, track=True)
    history, checked = [], []
    for call, k in enumerate((3, 70, 130)):
        its = (0, 1, k - 1)
        vals = reference_values(ref, sc, lambda: LibSim(pkg, sc, ref), history, list(its))
        tr.step(k)
        r_dev, s_dev, n = tr.residuals()[0]
        assert n == k and r_dev.size == k
        for j in its:
            v = vals[j]
            checked.append(("c%d.j%d" % (call + 1, j), v))
            e = [abs(np.longdouble(r_dev[j]) - v["r_u"]) / v["tol_r_u"], abs(np.longdouble(r_dev[j]) - v["r_dx"]) / v["tol_r_dx"], abs(np.longdouble(s_dev[j]) - v["s"]) / v["tol_s"]]
            print("growth step(%d) j %3d  r %.6e s %.6e  err/bound: r(u) %.3f  r(Dx) %.3f  s %.3f" % (k, j, r_dev[j], s_dev[j], e[0], e[1], e[2]))
            assert max(e) <= 1.0, (k, j, [float(q) for q in e])
        history.append(k)
    assert_sensitivity("growth", sc, checked)


@gpu
@pytest.mark.parametrize("mode", ["subtree", "contiguous"])
def test_two_shards(pkg, monkeypatch, mode):
    """two ranks on one GPU: |r|^2 is additive over the ranks' elements, s is summed over them before its norm; every rank reports the reference
    built from the union of the ranks' elements, bitwise the same on both"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    sc = bar_scene("TET_STVK", (3, 3, 20))
    gpu_case(pkg, "two shards %s" % mode, sc, world=2, mode=mode)


@gpu
@pytest.mark.parametrize("kind", sorted(KIND_SCENES) + ["mixed", "mixed_mesh"])
def test_tracking_is_neutral(pkg, monkeypatch, kind):
    """m_x, m_v, u and the warm-start state after two frames: bitwise the same with tracking on and off"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    sc = KIND_SCENES[kind]() if kind in KIND_SCENES else mixed_scene(kind == "mixed_mesh")
    ref = ResidualReference(make_oracle(sc))
    outs = []
    for track in (False, True):
        sim = LibSim(pkg, sc, ref, track=track)
        sim.step(5); sim.step(5)
        outs.append(sim.full())
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)


@gpu
@pytest.mark.parametrize("check_every", [1, 3])
@pytest.mark.parametrize("kind", ["TET_NH", "TET_STVK"])
def test_early_exit_at_the_iteration_the_reference_allows(pkg, monkeypatch, kind, check_every):
    """tol_r, tol_s between consecutive REFERENCE values (geometric means, at least 1000 derived bounds away from every value they separate):
    the loop ends after the first iteration j + 1 that is a multiple of check_every, not the last, with r_j <= tol_r and s_j <= tol_s"""
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    sc = KIND_SCENES[kind]()
    ref = ResidualReference(make_oracle(sc))
    iters = 5
    vals = reference_values(ref, sc, lambda: LibSim(pkg, sc, ref), [], [0, 1, 2, 3])
    r = [float(vals[j]["r_u"]) for j in range(4)]; s = [float(vals[j]["s"]) for j in range(4)]

    def stop(tol_r, tol_s):
        for j in range(iters - 1):
            if (j + 1) % check_every == 0 and r[j] <= tol_r and s[j] <= tol_s:
                return j + 1
        return iters

    def separates(tol_r, tol_s):      # at least 1000 derived bounds away from every reference value
        return all(abs(r[j] - tol_r) >= 1000 * vals[j]["tol_r_u"] and abs(s[j] - tol_s) >= 1000 * vals[j]["tol_s"] for j in range(4))
    # geometric means of consecutive reference values; the first pair that ends the loop inside the frame (reference values only decide)
    pairs = [(float(np.sqrt(r[a] * r[a + 1])), float(np.sqrt(s[b] * s[b + 1]))) for a in range(3) for b in range(3)]
    pairs = [p for p in pairs if separates(*p) and (1 < stop(*p) < iters)]
    assert pairs, (r, s)
    tol_r, tol_s = pairs[0]
    expected = stop(tol_r, tol_s)
    tr = LibSim(pkg, sc, ref, tolerance=(tol_r, tol_s, check_every))
    tr.step(iters)
    r_dev, s_dev, n = tr.residuals()[0]
    print("early exit %s check_every %d: r %s s %s tol %g %g -> expected %d, got %d" % (kind, check_every, r, s, tol_r, tol_s, expected, n))
    assert n == expected and r_dev.size == expected
