"""The frame prologue and epilogue (prologue_kernel, xbar_kernel, explicit_const_kernel, wind_serial_kernel, epilogue_kernel) against an
extended-precision reference.

Every case sets m_x and m_v to seeded values, runs step(0) -- the explicit forces, x_bar = x + dt v' and the epilogue, no ADMM iteration -- and
compares m_x (which is x_bar) and m_v (which is (x_bar - x) (1 / dt)) with checkers.explicit_reference: the reference's explicit loop in np.longdouble,
the forces in list order, the wind in serial triangle order.

The bound is derived (checkers.explicit_bound's docstring has the counts; nothing measured goes into it): two roundings per constant force on a node,
per wind triangle the roundings of its geometry, of v_r, v_n, the coefficient and the force carried through the serial chain (a triangle inherits a
third of its three nodes' bounds) plus one rounding per increment, two more for x_bar, and for v_out the subtraction, fl(1 / dt) and the product:
bound(x_bar) / dt + 3 EPS |v_out|, where the EPS |x_bar| / dt inside the first term dominates.  The derived wind term was NOT too optimistic for the
device or the oracle, so the 4 x-over-the-oracle fallback is not used.  For the record (CPU, the ordered list below): the float64 oracle and the
long-double loop differ by 0.93 bounds in v_out (bound 5.8e-15 at max |v'| = 8.7) and 0.93 bounds in x_bar (bound 2.3e-16: the rounding of x_bar
itself, EPS |x_bar| just above a power of two, is nearly the whole bound there).

The wind list: 2376 triangles over one node array in a seeded shuffle -- a 12 x 12 sym_plane cloth (576), 1500 node-disjoint triangles ("confetti")
and a 300-triangle fan around one hub node.  With the level rule of upload.inc restated here that is 300 dependency levels (the fan is a
serial chain through its hub) and a first level of 1540 triangles: wind_serial_kernel's strided loop takes a second trip.
"""
import functools
import itertools
import threading

import numpy as np
import pytest

from checkers import KIND, Oracle, explicit_bound, explicit_reference
from test_sharding import _thread_allreduce_hooks

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps > 2.0 ** -63, reason="np.longdouble has no extended precision on this host")
gpu = pytest.mark.gpu
DT = 0.04
WIND_A, WIND_B = (10.0, 0.0, 2.0), (-3.0, 4.0, 6.0)
GRAVITIES = [(0.0, -9.8, 0.0), (0.3, 0.0, -0.2), (-1.5, 0.25, 0.0), (0.0, 0.7, 0.9), (2.0, -0.1, 0.4)]


def _mg():
    from __graft_entry__ import load_package
    return load_package().meshgen


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict(x [n][3], v [n][3] seeded, tris [2376][3] shuffled, edges, hub)"""
    rng = np.random.default_rng(20240611)
    xc, tc = _mg().sym_plane(12, 12, size=1.0)
    xc = xc.copy(); xc[:, 1] = 0.1 * (xc[:, 0] * xc[:, 2])      # a wrinkle: the normals differ from triangle to triangle
    nc = xc.shape[0]
    cen = rng.uniform(0.0, 2.0, size=(1500, 1, 3)) + np.array([1.5, 0.0, 0.0])
    xf = (cen + 0.02 * rng.normal(size=(1500, 3, 3))).reshape(-1, 3)      # (small: the explicit drag of a larger triangle overshoots at these speeds)
    tf = nc + np.arange(4500, dtype=np.int32).reshape(-1, 3)
    hub = nc + 4500
    ang = 2.0 * np.pi * np.arange(300) / 300.0
    rim = np.stack([4.0 + 0.1 * np.cos(ang), 0.5 + 0.02 * np.cos(3.0 * ang), 0.1 * np.sin(ang)], axis=1)
    xh = np.concatenate([[[4.0, 0.55, 0.0]], rim])
    th = np.stack([np.full(300, hub), hub + 1 + np.arange(300), hub + 1 + (np.arange(300) + 1) % 300], axis=1).astype(np.int32)
    x = np.concatenate([xc, xf, xh])
    tris = np.concatenate([tc, tf, th]).astype(np.int32)
    tris = tris[rng.permutation(tris.shape[0])]
    assert tris.shape[0] == 2376
    n = x.shape[0]
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    chain = np.stack([np.arange(nc - 1, n - 1), np.arange(nc, n)], axis=1)      # joins the cloth, the confetti and the fan into one body
    edges = np.unique(np.sort(np.concatenate([e, chain]), axis=1), axis=0).astype(np.int32)
    return dict(x=x + 0.002 * rng.normal(size=x.shape), v=2.0 * rng.normal(size=x.shape), tris=tris, edges=edges, hub=int(hub), n=n,
                m3=np.full(3 * n, 1e-3), odd=np.arange(1, n, 2, dtype=np.int32))


def ordered_list(dir_a=WIND_A, g=GRAVITIES[0]):
    """a constant force on the odd nodes, wind, a gravity, a second wind with another direction over the list reversed, a constant force on an
    empty subset (which the reference and the library read as every node: ExplicitForce.cpp:30-32)"""
    sc = scene()
    return [("const", (0.5, 0.0, 0.2), sc["odd"]), ("wind", dir_a, sc["tris"]), ("const", g, None), ("wind", WIND_B, sc["tris"][::-1]),
            ("const", (0.0, 0.3, -0.1), np.zeros(0, np.int32))]


def wind_levels(tris, n):
    """the level rule of upload.inc: a triangle's level is one more than the highest level among earlier triangles sharing a node -> sizes per level"""
    last = np.zeros(n, np.int64); lev = np.zeros(tris.shape[0], np.int64)
    for t, q in enumerate(tris):
        lev[t] = 1 + last[q].max(); last[q] = lev[t]
    return np.bincount(lev)[1:]


def add_list(s, forces, pkg=None):
    """the explicit forces of `forces` on a library System (pkg given) or an Oracle -> their list indices"""
    which = []
    for type_, d, idx in forces:
        which.append(len(which))
        if type_ == "const" and idx is None:
            s.add_gravity(d)
        elif pkg is not None:
            s.add_explicit(pkg.EXPLICIT["CONST" if type_ == "const" else "WIND"], d, np.ascontiguousarray(idx, dtype=np.int32))
        else:
            s.add_explicit(0 if type_ == "const" else 1, d, np.ascontiguousarray(idx, dtype=np.int32))
    return which


def build(s, forces, pkg=None):
    sc = scene()
    s.add_nodes(sc["x"].ravel(), sc["m3"])
    s.add_forces(KIND["SPRING"], sc["edges"], [50.0])
    s.add_forces(KIND["ANCHOR"], np.array([0, 12], np.int32), [-1.0, 1.0])
    add_list(s, forces, pkg)
    return s


def compare(name, x, v, forces, x_out, v_out):
    """|x_out - x_bar| and |v_out - v_out_ref| against the derived bounds in every dof; prints the largest ratios -> the reference values"""
    (xb, vo, vp), (bx, bvo, bv) = explicit_bound(x, v, DT, forces)
    assert np.isfinite(x_out).all() and np.isfinite(v_out).all()
    rx, rv = np.abs(x_out.ravel() - xb) / bx, np.abs(v_out.ravel() - vo) / bvo
    print("%-40s max |v'| %.1f  largest error / bound: x_bar %.3f (bound %.2e)  v_out %.3f (bound %.2e)" %
          (name, float(np.abs(vp).max()), float(rx.max()), float(bx[np.argmax(rx)]), float(rv.max()), float(bvo[np.argmax(rv)])))
    assert rx.max() <= 1.0 and rv.max() <= 1.0, (name, float(rx.max()), float(rv.max()))
    return xb, vo, bx, bvo


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_wind_list_levels():
    sc = scene()
    sizes = wind_levels(sc["tris"], sc["n"])
    print("wind list: %d levels, the largest %d triangles" % (sizes.size, sizes.max()))
    assert sizes.size >= 300 and sizes.max() > 1024
    assert (sc["tris"] == sc["hub"]).any(axis=1).sum() == 300      # a 300-deep serial chain through one node


@pytest.mark.parametrize("which", ["wind", "ordered", "five gravities"])
def test_oracle_against_the_reference(which):
    """the oracle's explicit loop (float64, the same operations) stays within the bound derived for the kernels"""
    sc = scene()
    forces = dict(wind=[("wind", WIND_A, sc["tris"])], ordered=ordered_list())
    forces = forces[which] if which in forces else [("const", g, None) for g in GRAVITIES]
    o = build(Oracle(), forces); o.settings(DT, 0)
    assert o.initialize()
    o.x = sc["x"].ravel()
    o._view("v", o.dof)[:] = sc["v"].ravel()
    assert o.step()
    compare("oracle %s" % which, sc["x"], sc["v"], forces, o.x, o.v)


def test_order_matters_to_the_reference():
    """the reference in any other order of the last three (gravity, second wind, the all-node constant force) differs from the list's order by more
    than 1000 bounds: the comparison notices a swapped order"""
    sc = scene()
    forces = ordered_list()
    (xb, vo, vp), (bx, bvo, bv) = explicit_bound(sc["x"], sc["v"], DT, forces)
    for perm in itertools.permutations(range(2, 5)):
        if perm == (2, 3, 4):
            continue
        other = forces[:2] + [forces[i] for i in perm]
        xb2, vo2, _ = explicit_reference(sc["x"], sc["v"], DT, other)
        far = float((np.abs(vo2 - vo) / bvo).max())
        print("order %s: v_out differs by %.2e bounds" % (perm, far))
        assert far > 1000 and float((np.abs(xb2 - xb) / bx).max()) > 1000


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def lib_system(pkg, forces, rank=0, world=1):
    sc = scene()
    s = pkg.System(device_id=0); s.set_timestep(DT)
    build(s, forces, pkg)
    if world > 1:
        s.set_shard(rank, world); s.set_shard_mode("subtree")
    return s


def seeded(s, scale=1.0):
    sc = scene()
    s.m_x = sc["x"].ravel(); s.m_v = scale * sc["v"].ravel()


def frames(name, s, forces, scales=(1.0, -0.5)):
    """step(0) frames in ONE context, each from a seeded state (the positions, the velocities times `scale`: a state carried over from a frame of
    random velocities has stretched the triangles so far that the explicit drag overshoots and the frame after it overflows -- in the reference too)"""
    for f, scale in enumerate(scales):
        seeded(s, scale)
        x, v = s.m_x, s.m_v
        s.step(0)
        compare("%s frame %d" % (name, f + 1), x, v, forces, s.m_x, s.m_v)


@gpu
@pytest.mark.parametrize("count", [1, 4, 5])
def test_gravity_counts(pkg, count):
    """one gravity; four: the by-value table of prologue_kernel is full; five: the fifth moves the whole list to the general path, and all five
    must be applied"""
    forces = [("const", g, None) for g in GRAVITIES[:count]]
    s = lib_system(pkg, forces); s.initialize()
    frames("%d gravities" % count, s, forces)
    # a dropped force is visible: every one of them is worth more than 1000 bounds of v_out
    sc = scene()
    (xb, vo, vp), (bx, bvo, bv) = explicit_bound(sc["x"], sc["v"], DT, forces)
    for k in range(count):
        vo2 = explicit_reference(sc["x"], sc["v"], DT, forces[:k] + forces[k + 1:])[1]
        assert (np.abs(vo2 - vo) / bvo).max() > 1000


@gpu
def test_ordered_list(pkg):
    """a subset force, wind, a gravity, a second wind, an all-node force given as an empty subset: in list order (test_order_matters_to_the_reference:
    any other order is more than 1000 bounds away).  The wind's 2376 triangles: a second trip of the strided loop and a 300-deep chain"""
    forces = ordered_list()
    s = lib_system(pkg, forces); s.initialize()
    frames("ordered list", s, forces)


@gpu
@pytest.mark.parametrize("path", ["fast", "general"])
def test_set_gravity_after_initialize(pkg, monkeypatch, path):
    """fast path: two gravities, the second changed; general path: the first wind's direction and the gravity behind it changed.  The next step(0)
    matches the reference with the NEW values (the old ones are more than 1000 bounds away), and a step(5) frame after it is bitwise the same with
    and without the captured iteration graph"""
    sc = scene()
    if path == "fast":
        old = [("const", GRAVITIES[0], None), ("const", GRAVITIES[1], None)]
        new = [old[0], ("const", (0.0, 0.0, -3.0), None)]
        changes = [(1, (0.0, 0.0, -3.0))]
    else:
        old = ordered_list()
        new = ordered_list(dir_a=(0.0, 6.0, -8.0), g=(1.0, -2.0, 0.5))
        changes = [(1, (0.0, 6.0, -8.0)), (2, (1.0, -2.0, 0.5))]
    out = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("ADMM_HIP_GRAPH", graph)
        s = lib_system(pkg, old); s.initialize()
        seeded(s)
        for which, d in changes:
            s.set_gravity(which, d)
        s.step(0)
        x1, v1 = s.m_x, s.m_v
        if graph == "1":
            xb, vo, bx, bvo = compare("set_gravity %s" % path, sc["x"], sc["v"], new, x1, v1)
            vo_old = explicit_reference(sc["x"], sc["v"], DT, old)[1]
            assert (np.abs(vo_old - vo) / bvo).max() > 1000
        seeded(s, 0.25)      # (from slow velocities: see frames())
        s.step(5)
        out[graph] = (x1, v1, s.m_x, s.m_v, s.graph_state())
        assert np.isfinite(out[graph][2]).all()
    print("set_gravity %s: graph state with ADMM_HIP_GRAPH=1 %s, =0 %s" % (path, out["1"][4], out["0"][4]))
    for a, b in zip(out["1"][:4], out["0"][:4]):
        assert np.array_equal(a, b)


@gpu
def test_ordered_list_on_two_subtree_shards(pkg, monkeypatch):
    """every rank applies the whole list to its copy of the state: m_x and m_v of both ranks are bitwise those of one rank"""
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    forces = ordered_list()
    one = lib_system(pkg, forces); one.initialize()
    seeded(one); one.step(0)
    shards = [lib_system(pkg, forces, r, 2) for r in range(2)]
    for s, h in zip(shards, _thread_allreduce_hooks(2)):
        s.set_allreduce(h)
    pkg.initialize_together(shards)
    errs = []

    def run(r):
        try:
            seeded(shards[r]); shards[r].step(0)
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert not errs and not any(t.is_alive() for t in th), errs
    for s in shards:
        assert np.array_equal(s.m_x, one.m_x) and np.array_equal(s.m_v, one.m_v)
