"""Cloth self-collision (extension, no reference counterpart): a sheet surface whose own nodes meet it outside their 1-ring
(admm_hip_set_sheet_self_collision, project_collision_self_kernel, closest_within_excluding in csrc/mesh_query.hpp).

CPU: the host rule with a per-point excluded vertex against an np.longdouble brute force; skip_vertex = -1 bitwise Mesh.query; the
folded strip; the refusals.  GPU: the kernel bit-exact against the host composition; the flag off; two disconnected patches against
the closed form of a floor; launch modes, two shards, the class API; a cloth folding onto itself.

The folded strip is meshgen.folded_strip(4, 12, gap): sym_plane's topology, so its 5 x 13 grid vertices come with 48 cell-centre
vertices, 113 nodes in all (two 64-lane blocks, the second one partial)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from checkers import KIND
from test_collision_friction import DT, G, W
from test_collision_frames import IDENT, _frame, _rot
from test_collision_mesh import FLOOR, MESH, _closest_on_tris
from test_collision_shell import _capped_icosphere, _cube, _extent, _grid, _near_surface, _same_frames
from test_moving_friction import _np_rigid

L = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADMM_ERR_ARG, ADMM_ERR_STATE = 1, 3

SW, SL = 4, 12                        # the strip: 4 x 12 cells of size H
H = 0.25
NV_GRID = (SW + 1) * (SL + 1)         # 65 grid vertices, then 48 centre vertices
R_HOST = 0.1875                       # the half thickness of the host-rule tests: above the 1-ring's reach on all three meshes, so own vertices hit
R_STRIP = 0.1875                      # 3 H / 4: the vertices of the grid row before the fold are 0.545 H from the nearest triangle outside their 1-ring
GAP_STRIP = 0.03125                   # H / 8 < R_STRIP


def _strip(pkg, gap):
    V, F = pkg.meshgen.folded_strip(SW, SL, gap)
    return np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)


def _flaps(gap):
    """-> (lower, upper) boolean masks over the strip's vertices by their arc length (folded_strip's docstring); for gap < 7 H / 16 every
    vertex is on one of them"""
    jj = np.concatenate([np.repeat(np.arange(SL + 1.0), SW + 1), np.repeat(np.arange(SL) + 0.5, SW)])
    s = jj / SW
    a = (SL // 2 + 0.0625) / SW
    return s <= a, s > a + gap


def _host_meshes(pkg):
    return {"grid": _grid(), "strip": _strip(pkg, GAP_STRIP), "capped_ico": _capped_icosphere()}


def _brute_excluding(V, F, P, skip):
    """np.longdouble: for every point the two smallest distances over all triangles that do not have skip[i] as a corner, the winner
    (ties to the lowest index) and its closest point -> (c, d, tri, d_second); d = inf where every triangle is left out"""
    Vl, Pl = V.astype(L), P.astype(L)
    npt, nt = len(P), len(F)
    A, B, C = Vl[F[:, 0]], Vl[F[:, 1]], Vl[F[:, 2]]
    cp = _closest_on_tris(np.repeat(Pl, nt, 0), np.tile(A, (npt, 1)), np.tile(B, (npt, 1)), np.tile(C, (npt, 1))).reshape(npt, nt, 3)
    d2 = ((cp - Pl[:, None, :]) ** 2).sum(2)
    out = (F[None, :, :] == np.asarray(skip)[:, None, None]).any(2)
    d2 = np.where(out, L(np.inf), d2)
    tri = d2.argmin(1)
    best = d2[np.arange(npt), tri]
    d2b = d2.copy(); d2b[np.arange(npt), tri] = L(np.inf)
    return cp[np.arange(npt), tri], np.sqrt(best), tri, np.sqrt(d2b.min(1))


def _host_points(V, F, r, seed):
    """the mesh's own vertices displaced by a seeded field of up to about r / 2, each with its own id, then points near the surface
    with nothing left out"""
    rng = np.random.default_rng(seed)
    own = V + rng.uniform(-0.5 * r, 0.5 * r, V.shape)
    free = _near_surface(V, F, r, seed + 1, 400)
    P = np.ascontiguousarray(np.concatenate([own, free]))
    skip = np.concatenate([np.arange(len(V)), np.full(len(free), -1)]).astype(np.int32)
    return P, skip


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: the host rule against a brute force
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "strip", "capped_ico"])
def test_host_rule_excluding_vs_longdouble(pkg, name):
    """Mesh.query_excluding against the np.longdouble minimum over all triangles that do not have skip_vertex as a corner, with the
    bounds of the shell row of DESIGN section 4: the decision exact wherever |d - r| > 1e-9 extent; proj within
    1e-12 (extent + |q|) (1 + r / d); the winning triangle equal wherever the two best distances differ by more than 1e-9 extent.
    At most 1 % of the points may be left out by the two margins (asserted; measured: 0 on the grid and the icosphere, 0.0097 on the
    strip: the five vertices of the grid row before the fold, whose two nearest outside triangles share their closest point, a vertex --
    an exact tie whatever the seed)."""
    V, F = _host_meshes(pkg)[name]
    r = R_HOST
    ext = _extent(V)
    m = pkg.Mesh(V, F, r)
    t = np.array([0.25, -0.5, 1.0])
    P0, skip = _host_points(V, F, r, {"grid": 101, "strip": 103, "capped_ico": 202}[name])
    P = np.ascontiguousarray(P0 + t)
    q = P - t
    proj, sd, tri = m.query_excluding(P, skip, t)
    c_ref, d_ref, tri_ref, d_2nd = _brute_excluding(V, F, q, skip)
    d64 = d_ref.astype(np.float64)
    hit_ref = d64 < r
    sure = np.abs(d64 - r) > 1e-9 * ext
    clear = ~hit_ref | ((d_2nd - d_ref).astype(np.float64) > 1e-9 * ext)
    excluded = 1.0 - (sure & clear).mean()
    print("%s: %d points (%d own vertices), share left out by the margins %.4f" % (name, len(P), len(V), excluded))
    assert excluded <= 0.01, excluded
    hit = (proj != P).any(1)
    assert np.array_equal(hit[sure], hit_ref[sure])
    own = skip >= 0
    assert (hit & own).sum() >= len(V) // 2 and (hit & ~own).sum() >= 50, ((hit & own).sum(), (hit & ~own).sum())
    assert np.array_equal(sd > 0, hit) and np.array_equal(proj[~hit], P[~hit])
    k = hit & sure & clear
    assert np.array_equal(tri[k], tri_ref[k])
    assert not (F[tri[hit & own]] == skip[hit & own, None]).any()                     # never a triangle of the excluded 1-ring
    first = 1e-12 * (ext + np.linalg.norm(q, axis=1))
    want = c_ref + (L(r) / d_ref)[:, None] * (q.astype(L) - c_ref) + t.astype(L)
    k = k & (d64 > 0)
    e_p = np.linalg.norm((proj.astype(L) - want).astype(np.float64), axis=1)[k] / (first[k] * (1 + r / d64[k]))
    e_sd = np.abs(sd[k] - (r - d64[k])) / first[k]
    print("%s: %d colliding (%d own), worst error / bound: proj %.3g, sdist %.3g" % (name, hit.sum(), (hit & own).sum(), e_p.max(), e_sd.max()))
    assert e_p.max() <= 1.0 and e_sd.max() <= 1.0, (e_p.max(), e_sd.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: nothing left out is Mesh.query
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "strip", "capped_ico"])
def test_skip_minus_one_is_mesh_query(pkg, name):
    """skip_vertex = -1 everywhere: proj and sdist bitwise Mesh.query's, with and without a frame, and the winning triangle that of the
    bounded search (Mesh.closest); on the grid with the bounded-search test's tie inputs, points equidistant from several triangles"""
    V, F = _host_meshes(pkg)[name]
    P, _ = _host_points(V, F, R_HOST, 111)
    if name == "grid":
        mid = 0.5 * (V[F[:, 1]] + V[F[:, 2]])
        P = np.concatenate([P, V + [0, 0.03125, 0], V - [0, 0.015625, 0], mid + [0, 0.03125, 0]])
    none = np.full(len(P), -1, np.int32)
    f = _frame(_rot([0.3, 1.0, -0.2], 0.7), [0.1, -0.2, 0.3])
    for r in (R_HOST, 0.25 * R_HOST):
        m = pkg.Mesh(V, F, r)
        for t in (np.zeros(3), np.array([0.25, -0.5, 1.0])):
            for frame in (None, IDENT, f):
                a = m.query(P + t, t, frame=frame)
                b = m.query_excluding(P + t, none, t, frame=frame)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, r, frame is None)
                c = m.query_excluding(P + t, -1, t, frame=frame)
                assert np.array_equal(b[0], c[0]) and np.array_equal(b[2], c[2])
        h = m.closest(P, r * r)
        box = ((m.info()["lo"] - r < P) & (P < m.info()["hi"] + r)).all(1)
        assert np.array_equal(m.query_excluding(P, none)[2], np.where(box, h["tri"], -1))
        assert (h["tri"] >= 0).sum() >= 50


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the folded strip
# ---------------------------------------------------------------------------------------------------------------------------------
def test_folded_strip_meets_its_other_flap(pkg):
    """folded_strip(4, 12, H / 8) with r = 3 H / 4: every vertex queried with its own id hits a triangle that has a corner on the other
    flap and none of its own 1-ring; queried with -1 it hits its own 1-ring at d2 == 0 (sdist == r exactly)"""
    V, F = _strip(pkg, GAP_STRIP)
    assert V.shape == (NV_GRID + SW * SL, 3) and np.array_equal(F, pkg.meshgen.sheet_tris(SW, SL))
    lower, upper = _flaps(GAP_STRIP)
    assert (lower | upper).all() and lower.sum() == 5 * 7 + 4 * 6
    assert np.array_equal(V[lower, 1], np.zeros(lower.sum())) and np.array_equal(V[upper, 1], np.full(upper.sum(), GAP_STRIP))
    m = pkg.Mesh(V, F, R_STRIP)
    ids = np.arange(len(V), dtype=np.int32)
    proj, sd, tri = m.query_excluding(V, ids)
    assert (tri >= 0).all() and (sd > 0).all() and (proj != V).any(1).all()
    assert not (F[tri] == ids[:, None]).any()
    other = np.where(lower[:, None], upper[F[tri]], lower[F[tri]]).any(1)
    assert other.all(), np.flatnonzero(~other)
    proj, sd, tri = m.query_excluding(V, -1)
    assert (F[tri] == ids[:, None]).any(1).all()
    assert np.array_equal(sd, np.full(len(V), R_STRIP))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 4: refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(pkg, rc, words, fn, *args):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*args)
    msg = str(e.value)
    assert ("error %d" % rc) in msg or ("code %d" % rc) in msg or (" %d:" % rc) in msg or (" %d " % rc) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _host_sheet(pkg, r, self_collision=None):
    """a host-only context: the flat 4 x 4 grid as a cloth (spacing 0.25), a closed tet block, an obstacle cube"""
    mg = pkg.meshgen
    V, F = _grid()
    xb, tets = mg.bar(1, 1, 1)
    xb = xb + [0.0, 1.0, 0.0]
    x = np.concatenate([V, xb])
    s = pkg.System(device_id=-1)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TRI_STRAIN"], F, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["TET_LINEAR"], tets + len(V), [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.sheet = s.add_sheet_surface(0, len(V), F, r) if self_collision is None else s.add_sheet_surface(0, len(V), F, r, self_collision=self_collision)
    s.body = s.add_body_surface(len(V), len(xb), mg.tet_surface(tets) + len(V))
    Vc, Fc = _cube()
    s.cube = s.add_collision_mesh(Vc + [3.0, 0, 0], Fc)
    s.set_collision_shapes([MESH, MESH, MESH], [[0, 0, 0, s.sheet], [0, 0, 0, s.body], [0, 0, 0, s.cube]])
    return s


def test_self_collision_refusals(pkg):
    s = _host_sheet(pkg, 0.125)
    _refused(pkg, ADMM_ERR_ARG, ["collision mesh %d" % s.cube, "obstacle mesh"], s.set_sheet_self_collision, s.cube, True)
    _refused(pkg, ADMM_ERR_ARG, ["collision mesh %d" % s.body, "closed body surface"], s.set_sheet_self_collision, s.body, True)
    _refused(pkg, ADMM_ERR_ARG, ["not a registered mesh"], s.set_sheet_self_collision, 9, True)
    s.set_sheet_self_collision(s.sheet, True)
    s.set_sheet_self_collision(s.sheet, False)
    s.set_sheet_self_collision(s.sheet, True)
    assert s.collision_form() == 5
    s.initialize()                                                                   # r = 0.125 = half the spacing: clear of itself
    _refused(pkg, ADMM_ERR_STATE, ["before finalize"], s.set_sheet_self_collision, s.sheet, False)
    # r above the grid spacing: vertex 0 lies 0.25 / sqrt(2) from triangle 1 = (1, 5, 6), across the first cell's diagonal
    s = _host_sheet(pkg, 0.3, self_collision=True)
    _refused(pkg, ADMM_ERR_ARG, ["sheet surface %d" % s.sheet, "vertex 0", "triangle 1", "0.176777", "half thickness 0.3"], s.initialize)
    s = _host_sheet(pkg, 0.3)                                                        # the same sheet without the flag finalizes
    assert s.collision_form() == 4
    s.initialize()
    # the limit itself: h / sqrt(2) = 0.1768 on this grid of spacing h = 0.25
    s = _host_sheet(pkg, 0.17, self_collision=True); s.initialize()
    s = _host_sheet(pkg, 0.18, self_collision=True)
    _refused(pkg, ADMM_ERR_ARG, ["vertex", "triangle", "0.176777"], s.initialize)
    # the context-free query
    Vc, Fc = _cube()
    P = np.zeros((3, 3))
    with pytest.raises(pkg.AdmmHipError):
        pkg.Mesh(Vc, Fc).query_excluding(P, -1)                                      # a closed mesh
    V, F = _grid()
    m = pkg.Mesh(V, F, 0.125)
    m.query_excluding(P, [len(V) - 1, -1, 0])
    for bad in (len(V), -2):
        with pytest.raises(pkg.AdmmHipError):
            m.query_excluding(P, [0, bad, -1])
        with pytest.raises(pkg.AdmmHipError):
            m.velocity_query_excluding(P, [0, bad, -1], np.zeros_like(V))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 5: the kernel against the host composition
# ---------------------------------------------------------------------------------------------------------------------------------
R_K = 0.09375         # the kernel scene: 3 H / 8, flaps H / 2 apart at rest (clear of each other: finalize accepts it)
GAP_K = 0.125
N_FREE = 17           # free particles behind the strip's 113 nodes: they meet the sheet with nothing left out
CUBE_T = np.array([0.2, 0.05, 0.4])


def _kernel_scene(pkg):
    """-> (x0 [130][3], F, skip [130], disp [130][3]): the strip at rest, free particles around it; a seeded displacement field that
    sends lower-flap nodes up and upper-flap nodes down by up to 0.11 (some cross towards the other flap, some stay clear)"""
    V, F = _strip(pkg, GAP_K)
    rng = np.random.default_rng(121)
    free = np.stack([rng.uniform(-0.6, 0.6, N_FREE), rng.uniform(-0.1, 0.25, N_FREE), rng.uniform(-0.1, 1.6, N_FREE)], 1)
    x0 = np.concatenate([V, free])
    up = np.where(V[:, 1] < 0.5 * GAP_K, 1.0, -1.0)
    disp = 0.01 * rng.normal(size=x0.shape)
    disp[:len(V), 1] += up * rng.uniform(0.0, 0.11, len(V))
    skip = np.concatenate([np.arange(len(V)), np.full(N_FREE, -1)]).astype(np.int32)
    return x0, F, skip, disp


def _kernel_lists(framed):
    """entries (type, params, frame, mu): [floor, the sheet itself (mesh 0), a closed cube obstacle (mesh 1)] and 64 entries cycling
    through them with the floor's height and the cube's place varied; framed: the floors tilted and the cubes turned"""
    rng = np.random.default_rng(122)
    fl = _frame(_rot([1.0, 0.0, 0.3], 0.05), [0.0, 0.02, 0.7]) if framed else IDENT.copy()
    fc = _frame(_rot([0.2, 1.0, -0.4], 0.8), CUBE_T + [0.02, 0.0, -0.03]) if framed else IDENT.copy()
    short = [(FLOOR, [0.0, 0.02, 0.0, 0.0], fl, 0.3), (MESH, [0.0, 0.0, 0.0, 0.0], IDENT.copy(), 0.0), (MESH, [*CUBE_T, 1.0], fc, 0.7)]
    full = []
    for k in range(64):
        ty, par, f, mu = short[k % 3]
        par, f = list(par), f.copy()
        d = rng.uniform(-0.15, 0.15, 3)
        if k >= 3 and k % 3 == 0:
            par[1] += 0.05 * d[1]
        if k >= 3 and k % 3 == 2:
            par[:3] = np.asarray(par[:3]) + d * [1, 0.3, 3]
            f[9:] += d * [1, 0.3, 3]
        full.append((ty, par, f, [0.3, 0.0, 0.7, np.inf, 0.15][k % 5] if k % 3 != 1 else 0.0))
    return {"short": short, "full": full}


def _kernel_compose(pkg, entries, sheet, cube, skip, p, x0, friction, mu_s, vel):
    """the list on the host in its order: shape_query, Mesh.query_excluding for the sheet (the nodes' own vertex ids), Mesh.query for
    the cube; with friction the moving rule after every entry that moved a point, the sheet's with its own coefficient and its nodes'
    frame-start v interpolated at the winning triangle -> (z, rows the sheet entries moved)"""
    by_sheet = np.zeros(len(p), bool)
    for ty, par, f, mu in entries:
        vi = np.zeros_like(p)
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            moved = moved.astype(bool)
        elif int(par[3]) == 0:
            q, sd, tri = sheet.query_excluding(p, skip, par[:3])
            moved = sd > 0                                                               # (a point at d = r - 1 ulp may be "pushed" onto its own bits)
            k = moved & (skip >= 0)
            assert np.array_equal(q[~moved], p[~moved]) and not (sheet.F[tri[k]] == skip[k, None]).any()
            by_sheet |= (q != p).any(1)
            mu = mu_s
            if friction:
                vi, _, ids = sheet.velocity_query_excluding(p, skip, vel, par[:3])
                assert (ids[moved] >= 0).all()
        else:
            proj, sd = cube.query(p, par[:3], frame=f)
            moved = sd > 0
            q = np.where(moved[:, None], proj, p)
        if friction and mu > 0:
            w = _np_rigid(np.zeros(9), q) + DT * vi
            q2, _ = pkg.friction_query_moving(p, q, x0, w, mu)
            q = np.where(moved[:, None], q2, q)
        p = q
    return p, by_sheet


def _kernel_system(pkg, entries, x0, F, self_collision, mu_s=0.0):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    n = len(x0)
    s.add_nodes(x0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    nv = n - N_FREE
    if self_collision is None:
        mid = s.add_sheet_surface(0, nv, F, R_K)
    else:
        mid = s.add_sheet_surface(0, nv, F, R_K, self_collision=self_collision)
    Vc, Fc = _cube()
    assert mid == 0 and s.add_collision_mesh(0.3 * Vc, Fc) == 1
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    s.set_collision_friction([e[3] if mu_s else 0.0 for e in entries])
    if mu_s:
        s.set_body_surface_friction(mid, mu_s)
    s.initialize()
    s.set_collision_frames([e[2] for e in entries])
    return s, b


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "surface_friction", "framed"])
@pytest.mark.parametrize("which", ["short", "full"])
def test_self_kernel_equals_host_composition(pkg, which, case):
    """the folded strip (113 nodes: two 64-lane blocks) and 17 free particles, one collision element per node, the list [floor, the
    sheet itself, a closed cube] or 64 entries of them: z and u bitwise the host composition.  plain and framed: one local step of the
    batch alone on candidates x0 + disp (admm_hip_local_step_only; the surface as finalize built it).  surface_friction: the sheet
    with a coefficient of its own, the nodes started with v = disp / dt, one frame of one iteration, so that the candidates are
    x0 + dt v, the surface is the frame-start one and its vertices carry the nodes' v.  On the parent commit the sheet's nodes skip
    their own surface; here at least a fifth of them are moved by it in the expected arrays (asserted)."""
    friction, framed = case == "surface_friction", case == "framed"
    x0, F, skip, disp = _kernel_scene(pkg)
    entries = _kernel_lists(framed)[which]
    nv = len(x0) - N_FREE
    mu_s = 0.5 if friction else 0.0
    rng = np.random.default_rng(123)
    u = np.where((rng.uniform(size=len(x0)) < 0.5)[:, None], 0.001, 0.01) * rng.normal(size=x0.shape)
    sheet = pkg.Mesh(x0[:nv], F, R_K); sheet.F = F
    Vc, Fc = _cube()
    cube = pkg.Mesh(0.3 * Vc, Fc)
    s, b = _kernel_system(pkg, entries, x0, F, True, mu_s)
    assert s.collision_form() == 5
    s.write_local(b, u=u)
    if friction:
        v = disp / DT
        sheet.set_vertices(x0[:nv])                                                  # (the arithmetic of the device's frame-start update)
        dx = x0 + DT * v
        s.m_v = v.ravel()
        s.step(1)
        assert s.body_surface_status(0) == dict(updated=1, refused=0, last_bad_tri=-1)
    else:
        v = np.zeros_like(x0)
        dx = x0 + disp
        s.local_step_dx(b, dx)
    want, by_sheet = _kernel_compose(pkg, entries, sheet, cube, skip, dx + u, x0, friction, mu_s, v[:nv])
    r = s.read_local(b)
    own = by_sheet[:nv].sum()
    print("%s list, %s: the sheet moves %d of its own %d nodes and %d of %d free particles" % (which, case, own, nv, by_sheet[nv:].sum(), N_FREE))
    assert own >= nv / 5 and by_sheet[nv:].sum() >= 2
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.flatnonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    if friction:
        still, _ = _kernel_compose(pkg, entries, sheet, cube, skip, dx + u, x0, True, mu_s, np.zeros_like(v[:nv]))
        assert np.abs(still - want).max() > 1e-4                                     # the vertices' velocities matter


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 6: the flag off
# ---------------------------------------------------------------------------------------------------------------------------------
def _frames(s, frames, iters=10):
    out = []
    for _ in range(frames):
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


@pytest.mark.gpu
def test_flag_off_changes_nothing(pkg):
    """the kernel scene falling under its nodes' velocities for four frames: self_collision=False is bitwise a context built without the
    new call -- frames, collision_form 4, graph state; and a list that names no sheet (form 0) is the same whether the registered
    sheet self-collides or not, while naming the self-colliding sheet gives form 5 and other frames"""
    x0, F, skip, disp = _kernel_scene(pkg)
    entries = _kernel_lists(False)["short"]
    res = {}
    for key in (None, False, True):
        s, _ = _kernel_system(pkg, entries, x0, F, key)
        s.m_v = (disp / DT).ravel()
        res[key] = (_frames(s, 4), s.collision_form(), s.graph_state())
    assert res[None][1] == res[False][1] == 4 and res[True][1] == 5
    assert _same_frames(res[None][0], res[False][0]) and res[None][2] == res[False][2], (res[None][2], res[False][2])
    assert res[None][2]["frame_graph_iters"] == 10
    assert not _same_frames(res[None][0], res[True][0])
    bare = [e for e in entries if not (e[0] == MESH and e[1][3] == 0.0)]
    out = {}
    for key in (None, True):
        s, _ = _kernel_system(pkg, bare, x0, F, key)
        s.m_v = (disp / DT).ravel()
        out[key] = (_frames(s, 4), s.collision_form(), s.graph_state())
    assert out[None][1] == out[True][1] == 0
    assert _same_frames(out[None][0], out[True][0]) and out[None][2] == out[True][2]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 7: two disconnected patches of one sheet, the closed form of a floor
# ---------------------------------------------------------------------------------------------------------------------------------
R_P = 0.125           # below 0.25 / sqrt(2), the rest-pose limit on this grid
C_P = 2.0             # the upper patch's speed: C_P * DT = 0.04 < R_P, the no-crossing condition
M_P = 0.5             # the nodes' mass: a candidate sinks M v / (dt w^2) = 0.5 * 2 / (0.02 * 1024) = 0.049 < R_P below the contact


def _patches():
    """one surface of two 3 x 3-cell square patches (cells of 0.25): the lower one at y = 0, the upper one at y = 3 r"""
    V, F = _grid(3, 0.75)
    up = V + [0.0, 3 * R_P, 0.0]
    return np.concatenate([V, up]), np.concatenate([F, F + len(V)]).astype(np.int32), len(V)


def _patch_run(pkg, listed, self_collision, frames=20, iters=20):
    x, F, nl = _patches()
    n = len(x)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.full(3 * n, M_P))
    s.add_forces(KIND["COLLISION"], np.arange(nl, n, dtype=np.int32), [W])
    mid = s.add_sheet_surface(0, n, F, R_P, self_collision=self_collision)
    if listed == "sheet":
        s.set_collision_shapes([MESH], [[0, 0, 0, mid]])
    else:
        s.set_collision_shapes([FLOOR], [[0, R_P if listed == "floor" else -100.0, 0, 0]])
    s.initialize()
    v = np.zeros_like(x); v[nl:, 1] = -C_P
    s.m_v = v.ravel()
    xs, vs = [], []
    for _ in range(frames):
        s.step(iters)
        xs.append(s.m_x.reshape(-1, 3).copy()); vs.append(s.m_v.reshape(-1, 3).copy())
    return np.array(xs), np.array(vs), s.collision_form(), s.body_surface_status(mid), nl


@pytest.mark.gpu
def test_two_patches_follow_the_floor_recursion(pkg):
    """no gravity, no elastic forces; the upper patch's 16 nodes start at y = 3 r with v = (0, -2, 0) and alone carry collision elements,
    the lower patch never moves; r = 0.125 is above the travel per frame (0.04) and above the sinking of a candidate below the
    contact (0.049), so no candidate crosses the mid-surface.  With self-collision on they follow, to 1e-9 over 20 frames x 20 iterations
    (the bound of the shell row: free particles over a sheet), the same nodes over a floor at y = r; with it off they are bitwise in free fall through y = 0.
    Measured on the MI355X: |x - floor| 8.6e-15, |v - floor| 3.3e-14, last height 1.000019 r; the lower patch moved by at most 1.28e-14."""
    xs, vs, form, st, nl = _patch_run(pkg, "sheet", True)
    xf, vf, _, _, _ = _patch_run(pkg, "floor", False)
    xo, vo, form_off, _, _ = _patch_run(pkg, "sheet", False)
    xc, vc, _, _, _ = _patch_run(pkg, "none", False)
    assert form == 5 and form_off == 4 and st == dict(updated=20, refused=0, last_bad_tri=-1)
    ex, ev = np.abs(xs[:, nl:] - xf[:, nl:]).max(), np.abs(vs[:, nl:] - vf[:, nl:]).max()
    print("two patches: |x - floor| %.3g, |v - floor| %.3g; last height / r %.6f" % (ex, ev, xs[-1, nl:, 1].min() / R_P))
    assert ex <= 1e-9 and ev <= 1e-9, (ex, ev)
    assert np.abs(xs[-1, nl:, 1] - R_P).max() < 1e-3                                  # they rest on the lower patch's upper face
    still = np.abs(xs[:, :nl] - _patches()[0][:nl]).max()                             # ... which never moved: no force, no velocity; each frame's
    print("two patches: the lower patch moved by at most %.3g" % still)               # solve of M x = M x returns x to a few ulps of 0.375
    assert still <= 20 * 16 * np.finfo(np.float64).eps * 0.375                        # 20 frames, 16 roundings of |x| <= 0.375 allowed in each (measured on the MI355X: 1.28e-14)
    assert np.array_equal(xo, xc) and np.array_equal(vo, vc)                          # off: free fall, bitwise
    assert np.abs(xo[-1, nl:, 1] - (3 * R_P - 20 * C_P * DT)).max() < 1e-12 and xo[-1, nl:, 1].max() < -3 * R_P


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 8 and 9: a cloth folding onto itself; launch modes, shards, the class API
# ---------------------------------------------------------------------------------------------------------------------------------
R_C = 0.078125        # 5 H / 16: the largest of the values tried that the fold's chord triangles leave clear at rest (3 H / 8 is refused at finalize); the flaps start 3 r apart
GAP_C = 3 * R_C


def _fold_scene(pkg):
    """the folded strip as a cloth: -> (x, m, F, hinges, anchors, upper): the lower flap's nodes (y == 0) anchored, the upper flap's
    (y == gap) free to fall"""
    V, F = _strip(pkg, GAP_C)
    return V, np.full(len(V), 0.02), F, pkg.meshgen.bend_hinges(F), np.flatnonzero(V[:, 1] == 0.0).astype(np.int32), V[:, 1] == GAP_C


def _fold_system(pkg, self_collision, rank=0, world=1, mode=None, mu=0.0):
    x, m, F, hinges, anch, _ = _fold_scene(pkg)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TRI_STRAIN"], F, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["BEND"], hinges, [20.0])
    s.add_forces(KIND["ANCHOR"], anch, [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    if world > 1:
        s.set_shard(rank, world)
        if mode:
            s.set_shard_mode(mode)
    s.mid = s.add_sheet_surface(0, len(x), F, R_C, self_collision=self_collision)
    if mu:
        s.set_body_surface_friction(s.mid, mu)
    s.set_collision_shapes([MESH], [[0, 0, 0, s.mid]])
    return s


@pytest.mark.gpu
def test_cloth_folds_onto_itself(pkg):
    """the folded strip as a cloth (LimitedTriangleStrain + BendForce), the lower flap anchored, the upper flap released 3 r above it
    under gravity, 40 frames of 10 iterations.  r = 0.078 is above closing speed x dt (a fall of 2 r: sqrt(2 g 2 r) dt = 0.035) and above
    the sinking M v / (dt w^2) = 0.02 * 1.75 / (0.02 * 1024) = 0.002.  With self-collision on no upper-flap node's height above the lower
    flap's plane changes sign and no frame is refused; with it off at least one node crosses.  The resting gap (the lowest upper-flap
    node's height / r) is printed, no bound asserted on it.  Measured on the MI355X: resting gap 0.9999 r, lowest ever 0.9988 r, largest
    |v_y| 1.60 (0.032 of travel a frame); with the flag off the lowest node reaches -17.2 r."""
    _, _, _, _, _, upper = _fold_scene(pkg)
    out = {}
    for on in (True, False):
        s = _fold_system(pkg, on); s.initialize()
        ys, vmax = [], 0.0
        for _ in range(40):
            s.step(10)
            ys.append(s.m_x.reshape(-1, 3)[upper, 1].copy())
            vmax = max(vmax, np.abs(s.m_v.reshape(-1, 3)[upper, 1]).max())
        out[on] = (np.array(ys), vmax, s.body_surface_status(s.mid), s.collision_form())
    ys, vmax, st, form = out[True]
    print("fold: resting gap %.4f r (lowest upper-flap node after 40 frames), lowest ever %.4f r, largest |v_y| %.3f; off: lowest %.4f r" %
          (ys[-1].min() / R_C, ys.min() / R_C, vmax, out[False][0].min() / R_C))
    assert form == 5 and out[False][3] == 4
    assert st == dict(updated=40, refused=0, last_bad_tri=-1) and out[False][2]["refused"] == 0
    assert (ys > 0).all()                                                            # no node crosses the lower flap's plane
    assert (out[False][0] < 0).any()                                                 # without self-collision some do


def _mode_results(pkg):
    s = _fold_system(pkg, True, mu=0.3); s.initialize()
    fr = _frames(s, 3)
    return dict(x=np.array([f[0] for f in fr]), v=np.array([f[1] for f in fr]))


def _child_main(path):
    from __graft_entry__ import load_package
    np.savez(path, **_mode_results(load_package()))


@pytest.mark.gpu
def test_self_collision_launch_modes_bitwise(pkg, monkeypatch, tmp_path):
    """three frames of the folding cloth (with a surface coefficient): eager, iteration graph, frame graph in this process and
    ADMM_HIP_LOCAL_MULTI=0 in a fresh child process give the same bits"""
    res = {}
    for env in ({}, {"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res[tuple(env.items())] = _mode_results(pkg)
    keys = list(res)
    for k in keys[1:]:
        for name, v in res[keys[0]].items():
            assert np.array_equal(res[k][name], v), (k, name)
    for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, ADMM_HIP_LOCAL_MULTI="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_sheet_self_collision as t; t._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.load(path)
    for name, v in res[keys[0]].items():
        assert np.array_equal(got[name], v), name
    assert np.abs(res[keys[0]]["x"][-1] - res[keys[0]]["x"][0]).max() > 1e-3


@pytest.mark.gpu
def test_self_collision_two_subtree_shards(pkg, monkeypatch):
    """the same three frames in two subtree shards (two contexts on one GPU): the ranks bitwise equal and within 1e-9 of one rank"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    ref = _fold_system(pkg, True, mu=0.3); ref.initialize()
    refx = _frames(ref, 3)
    shards = [_fold_system(pkg, True, rank=r, world=2, mode="subtree", mu=0.3) for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert all(s.collision_form() == 5 for s in shards)
    res, errs = [None, None], []

    def run(r):
        try:
            res[r] = _frames(shards[r], 3)
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    assert _same_frames(res[0], res[1])
    for f in range(3):
        d = np.abs(res[0][f][0] - refx[f][0]).max()
        assert d < 1e-9, (f, d)


def test_cpp_self_collision_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_self_collision", pkg))


@pytest.mark.gpu
def test_class_api_self_collision(pkg, tmp_path):
    """the folding cloth through admm::System with CollisionSheet::self_collision set: bitwise the C ABI's frames"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_self_collision", pkg)
    x, m, F, hinges, anch, _ = _fold_scene(pkg)
    frames, iters = 3, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(F), len(hinges), len(anch), 1], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (F, hinges, anch):
            np.asarray(a).astype(np.int32).tofile(f)
        np.array([R_C, DT, 0.3]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(outp).reshape(frames, 2, len(x) * 3)
    s = _fold_system(pkg, True, mu=0.3); s.initialize()
    want = _frames(s, frames, iters)
    for f in range(frames):
        assert np.array_equal(got[f, 0], want[f][0]) and np.array_equal(got[f, 1], want[f][1]), (f, np.abs(got[f, 0] - want[f][0]).max())
