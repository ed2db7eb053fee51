"""Open triangle surfaces as thick shells (admm_hip_mesh_create_open, admm_hip_add_sheet_surface, project_collision_shell_kernel).

On the CPU: validation, the host rule against an np.longdouble brute force and a float64 restatement of the documented order, the
bounded search against the unbounded one, updates, closed meshes against arrays recorded with the parent's library, the argument
checks.  On the GPU: the shell kernel bit for bit against a composition of the host routines, lists without an open mesh as before,
the thickness under a captured graph, the launch modes, device updates, free particles on a flat sheet against a floor, a sheet
surface that follows its cloth against the host-driven route, contact that a control lacks, and the conveyor check on a sheet.

No reference counterpart: the expected values come from numpy in here."""

import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from checkers import KIND
from conftest import golden
from test_collision_friction import DT, G, W, _expect, _kernel_case
from test_collision_frames import BOX, IDENT, _frame, _rot, _rotate, _to_local
from test_collision_mesh import FLOOR, MESH, _closest_on_tris, icosphere, mesh
from test_moving_friction import _np_rigid

L = np.longdouble
EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SHELL = 0.0625      # the half thickness of the test meshes (exactly representable)


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid(n=4, size=1.0):
    """an n x n-cell square sheet in the plane y = 0, normals +y, vertices at multiples of size / n"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    V = np.stack([i.ravel() * (size / n) - size / 2, np.zeros((n + 1) ** 2), j.ravel() * (size / n) - size / 2], 1)
    F = []
    for jj in range(n):
        for ii in range(n):
            a = jj * (n + 1) + ii; b = a + 1; c = a + n + 1; d = c + 1
            F += [[a, c, b], [b, c, d]]
    return V, np.array(F, dtype=np.int32)


def _quarter_cylinder():
    V, F = _grid()
    th = (V[:, 0] + 0.5) * (np.pi / 2)
    R = 2 / np.pi
    return np.stack([R * np.sin(th), R * (1 - np.cos(th)), V[:, 2]], 1), F


def _capped_icosphere():
    """icosphere(2) of radius 0.5 without the triangles around its top: one boundary loop"""
    V, F = icosphere(2, 0.5)
    F = F[V[F].mean(1)[:, 1] < 0.3]
    used = np.unique(F)
    new = np.full(len(V), -1); new[used] = np.arange(len(used))
    return np.ascontiguousarray(V[used]), new[F].astype(np.int32)


def _cube():
    V, F = mesh("cube")
    return V - 0.5, F


SHELLS = {
    "triangle": lambda: (np.array([[0.0, 0, 0], [1, 0, 0], [0, 0.5, 1]]), np.array([[0, 1, 2]], dtype=np.int32)),
    "square": lambda: _grid(1),
    "grid": _grid,
    "cylinder": _quarter_cylinder,
    "capped_ico": _capped_icosphere,
    "cube": _cube,
}


def _extent(V):
    return float((V.max(0) - V.min(0)).max())


def _brute(V, F, P):
    """the closest point of the surface to every point in np.longdouble, by exhaustive search -> (c, d, tri): ties to the lowest index"""
    V = V.astype(L); P = P.astype(L)
    npt, nt = len(P), len(F)
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    cp = _closest_on_tris(np.repeat(P, nt, 0), np.tile(A, (npt, 1)), np.tile(B, (npt, 1)), np.tile(C, (npt, 1))).reshape(npt, nt, 3)
    d2 = ((cp - P[:, None, :]) ** 2).sum(2)
    tri = d2.argmin(1)
    return cp[np.arange(npt), tri], np.sqrt(d2[np.arange(npt), tri]), tri


def _points(V, r, seed, n=1500):
    """random points in the root box inflated by 2 r, a fifth of them within 2 r of the surface, and some well beyond the box"""
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0), V.max(0)
    P = rng.uniform(lo - 2 * r, hi + 2 * r, (n, 3))
    far = rng.uniform(lo - 1.0, hi + 1.0, (n // 10, 3))
    return np.ascontiguousarray(np.concatenate([P, far]))


def _near_surface(V, F, r, seed, n=600):
    """points at a uniform distance in (0, 2 r) from random points of the surface along the face normal, both sides"""
    rng = np.random.default_rng(seed)
    f = F[rng.integers(0, len(F), n)]
    w = rng.dirichlet([1, 1, 1], n)
    base = (w[:, :, None] * V[f]).sum(1)
    nrm = np.cross(V[f[:, 1]] - V[f[:, 0]], V[f[:, 2]] - V[f[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return base + (rng.uniform(0, 2 * r, n) * np.where(rng.uniform(size=n) < 0.5, -1, 1))[:, None] * nrm


def _face_normal64(V, T):
    """the unit face normal as the library computes it: corners rotated so that the lowest vertex id comes first, cross, / sqrt(dot)"""
    k = int(np.argmin(T))
    a, b, c = V[T[k]], V[T[(k + 1) % 3]], V[T[(k + 2) % 3]]
    e1, e2 = b - a, c - a
    n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    return n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])


def _restate(m, V, F, r, P, t):
    """section 1 of the rule in plain float64 numpy on the library's own hit (Mesh.closest bounded by r * r) -> (proj, collides)"""
    q = P - t
    inf = m.info()
    box = ((inf["lo"] - r < q) & (q < inf["hi"] + r)).all(1)
    h = m.closest(q, r * r)
    hit = box & (h["slot"] >= 0) & (h["d2"] < r * r)
    out = P.copy()
    c, d2 = h["c"], h["d2"]
    for i in np.nonzero(hit)[0]:
        e = q[i] - c[i]
        d = np.sqrt(d2[i])
        if d > 0:
            s = r / d
            o = c[i] + s * e
        else:
            o = c[i] + r * _face_normal64(V, F[h["tri"][i]])
        out[i] = t + o
    return out, hit


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: validation
# ---------------------------------------------------------------------------------------------------------------------------------
def _open_error(pkg, V, F, r, *words):
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(V, F, r)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_open_mesh_validation(pkg):
    """accepted: a single triangle, boundary edges, a closed input; refused with the edge or triangle named: an edge with three faces,
    opposite winding across an edge, a degenerate triangle, a bad thickness; admm_hip_mesh_create refuses the open inputs as before"""
    for name, make in SHELLS.items():
        V, F = make()
        m = pkg.Mesh(V, F, R_SHELL)
        assert m.thickness == R_SHELL and m.info()["n_tris"] == len(F), name
    Vc, Fc = _cube()
    assert pkg.Mesh(Vc, Fc).thickness == 0.0
    V, F = _grid()
    fin = np.array([[F[0, 0], F[0, 1], len(V)]], np.int32)                           # a third face on the first triangle's interior edge (b, c)
    Vf = np.concatenate([V, [[0.0, 0.5, 0.0]]])
    F3 = np.concatenate([F, [[F[1, 0], F[1, 1], len(V)]]]).astype(np.int32)
    lo, hi = sorted((int(F[1, 0]), int(F[1, 1])))
    _open_error(pkg, Vf, F3, R_SHELL, "edge (%d, %d)" % (lo, hi), "shared by 3 triangles", "not edge-manifold")
    Fl = F.copy(); Fl[1] = Fl[1, [0, 2, 1]]
    _open_error(pkg, V, Fl, R_SHELL, "same direction", "triangles 0 and 1", "edge (%d, %d)" % (lo, hi))
    Vd = V.copy(); Vd[F[3, 2]] = 0.5 * (V[F[3, 0]] + V[F[3, 1]])
    bad = int(np.flatnonzero(np.linalg.norm(np.cross(Vd[F[:, 1]] - Vd[F[:, 0]], Vd[F[:, 2]] - Vd[F[:, 0]]), axis=1) == 0)[0])
    _open_error(pkg, Vd, F, R_SHELL, "triangle %d" % bad, "degenerate")
    _open_error(pkg, V, np.concatenate([F, [[3, 3, 7]]]).astype(np.int32), R_SHELL, "triangle %d" % len(F), "degenerate")
    for r in (0.0, -0.1, np.nan, np.inf):
        _open_error(pkg, V, F, r, "half thickness", "positive and finite")
    del fin
    # the closed route as before, with the same messages (test_collision_mesh.test_mesh_validation's)
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(Vc, Fc[1:])
    assert "open" in str(e.value) and "shared by 1 triangle" in str(e.value)
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(V, F)
    assert "open" in str(e.value) and "shared by 1 triangle" in str(e.value)
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(*SHELLS["triangle"]())
    assert "at least 4 vertices and 4 triangles" in str(e.value)
    with pytest.raises(pkg.AdmmHipError) as e:
        pkg.Mesh(Vc, Fc[:, [0, 2, 1]])
    assert "volume" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: the host rule against the longdouble brute force
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHELLS))
def test_host_rule_vs_longdouble(pkg, name):
    """random points in the inflated box, near the surface and beyond the box.  The decision equals the brute force's wherever
    |d_ref - r| > 1e-9 extent (at most 1 % of the points may be left out: asserted, 0 measured); proj within
    1e-12 (extent + |q|) (1 + r / d_ref) of the reference -- the closed-mesh test's bound on c times the conditioning of the
    direction (q - c) / d -- and for d_ref < r / 16 only | |proj - c_ref| - r | to the first factor; sdist = r - d to the first
    factor; unmoved points bitwise; the float64 restatement of the documented order on the winning triangle bitwise."""
    V, F = SHELLS[name]()
    r = R_SHELL
    ext = _extent(V)
    m = pkg.Mesh(V, F, r)
    t = np.array([0.25, -0.5, 1.0])
    P0 = np.concatenate([_points(V, r, 11), _near_surface(V, F, r, 12)])
    P = np.ascontiguousarray(P0 + t)
    q = P - t                                                                       # what the library sees
    proj, sd = m.query(P, t)
    c_ref, d_ref, _ = _brute(V, F, q)
    d64 = d_ref.astype(np.float64)
    sure = np.abs(d64 - r) > 1e-9 * ext
    excluded = 1.0 - sure.mean()
    assert excluded <= 0.01, excluded
    hit_ref = d64 < r
    hit = (proj != P).any(1)
    assert np.array_equal(hit[sure], hit_ref[sure])
    assert 100 <= hit.sum() <= len(P) - 100, hit.sum()
    assert np.array_equal(sd > 0, hit) and np.isneginf(sd[~hit]).all()
    first = 1e-12 * (ext + np.linalg.norm(q, axis=1))
    k = hit & sure
    e_sd = np.abs(sd[k] - (r - d64[k])) / first[k]
    assert e_sd.max() <= 1.0, e_sd.max()
    want = c_ref + (L(r) / d_ref)[:, None] * (q.astype(L) - c_ref) + t.astype(L)
    well = k & (d64 >= r / 16)
    e_p = np.linalg.norm((proj.astype(L) - want).astype(np.float64), axis=1)[well] / (first[well] * (1 + r / d64[well]))
    assert e_p.max() <= 1.0, e_p.max()
    close = k & (d64 < r / 16)
    e_c = np.abs(np.linalg.norm(((proj - t).astype(L) - c_ref).astype(np.float64), axis=1) - r)[close] / first[close] if close.any() else np.zeros(1)
    assert e_c.max() <= 1.0, e_c.max()
    assert np.array_equal(proj[~hit], P[~hit])                                      # unmoved: the same bits
    same, hit64 = _restate(m, V, F, r, P, t)
    assert np.array_equal(hit64, hit) and np.array_equal(same, proj)
    print("%s: %d points, %d colliding, excluded %.4f, worst error / bound: proj %.3g, sdist %.3g, near-surface %.3g" %
          (name, len(P), hit.sum(), excluded, e_p.max(), e_sd.max(), e_c.max()))


def test_points_on_the_surface(pkg):
    """d == 0: points on a face, an edge and a vertex of the flat grid (coordinates exactly representable) leave along the winning
    triangle's unit normal, +y: to y = r exactly; also under a translation and a frame (a quarter turn: exact)"""
    V, F = _grid()
    r = R_SHELL
    m = pkg.Mesh(V, F, r)
    P = np.array([[0.0625, 0.0, 0.03125], [0.125, 0.0, 0.0], [0.25, 0.0, -0.25], [-0.5, 0.0, -0.5], [0.5, 0.0, 0.125], [-0.3125, 0.0, 0.40625]])
    proj, sd = m.query(P)
    assert np.array_equal(sd, np.full(len(P), r))                                    # d == 0 exactly: the second branch
    want = P.copy(); want[:, 1] = r
    assert np.array_equal(proj, want)
    same, hit = _restate(m, V, F, r, P, np.zeros(3))
    assert hit.all() and np.array_equal(same, proj)
    t = np.array([0.5, 0.25, -1.0])
    proj, sd = m.query(P + t, t)
    assert np.array_equal(proj, want + t) and np.array_equal(sd, np.full(len(P), r))
    f = _frame(np.round(_rot([0, 0, 1.0], np.pi / 2)), [0.0, 0.0, 0.0])               # local y -> world -x
    Pw = np.stack([-P[:, 1], P[:, 0], P[:, 2]], 1)
    proj, sd = m.query(Pw, (0.0, 0.0, 0.0), frame=f)
    assert np.array_equal(proj, np.stack([-want[:, 1], want[:, 0], want[:, 2]], 1)) and np.array_equal(sd, np.full(len(P), r))
    # the faces of the inflated box and d2 == r * r are not collisions: strict comparisons
    edge = np.array([[0.0, r, 0.0], [0.0, -r, 0.0], [0.5 + r, 0.0, 0.0], [-0.5 - r, 0.03125, 0.125], [0.25, 0.03125, 0.5 + r]])
    proj, sd = m.query(edge)
    assert np.array_equal(proj, edge) and np.isneginf(sd).all()
    inside = np.array([[0.0, 0.5 * r, 0.0], [0.0, -0.5 * r, 0.0], [0.5 + 0.5 * r, 0.0, 0.0]])
    proj, sd = m.query(inside)
    assert np.array_equal(proj, np.array([[0.0, r, 0.0], [0.0, -r, 0.0], [0.5 + r, 0.0, 0.0]])) and np.array_equal(sd, np.full(3, 0.5 * r))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the bounded search is the unbounded one below r
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "capped_ico"])
def test_bounded_search_equals_unbounded(pkg, name):
    """closest_within and closest: the same slot, region, c and d2, bitwise, wherever d2 < r^2, and no hit elsewhere; with points
    equidistant from several triangles (over vertices and edge midpoints of the grid), where the lowest index wins in both"""
    V, F = SHELLS[name]()
    m = pkg.Mesh(V, F, R_SHELL)
    P = np.concatenate([_points(V, R_SHELL, 21), _near_surface(V, F, R_SHELL, 22)])
    ties = np.zeros((0, 3))
    if name == "grid":
        mid = 0.5 * (V[F[:, 1]] + V[F[:, 2]])
        ties = np.concatenate([V + [0, 0.03125, 0], V - [0, 0.015625, 0], mid + [0, 0.03125, 0]])
        P = np.concatenate([P, ties])
    for r in (R_SHELL, 0.25 * R_SHELL, 3 * R_SHELL):
        a, b = m.closest(P), m.closest(P, r * r)
        near = a["d2"] < r * r
        assert 50 <= near.sum() <= len(P) - 50
        for k in ("slot", "reg", "c", "d2", "tri"):
            assert np.array_equal(a[k][near], b[k][near]), (k, r)
        assert (b["slot"][~near] == -1).all() and np.isinf(b["d2"][~near]).all()
    if name == "grid":
        a = m.closest(ties)
        _, _, tri = _brute(V, F, ties)
        cp_all = np.stack([_closest_on_tris(ties, V[F[k, 0]][None].repeat(len(ties), 0), V[F[k, 1]][None].repeat(len(ties), 0),
                                            V[F[k, 2]][None].repeat(len(ties), 0)) for k in range(len(F))], 1)
        d2_all = ((cp_all - ties[:, None, :]) ** 2).sum(2)
        n_tied = (d2_all == d2_all.min(1)[:, None]).sum(1)
        assert (n_tied >= 2).sum() >= 40                                             # exact ties are there
        lowest = np.array([np.flatnonzero(d2_all[i] == d2_all[i].min())[0] for i in range(len(ties))])
        assert np.array_equal(a["tri"], lowest)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 4: updates
# ---------------------------------------------------------------------------------------------------------------------------------
def _bend(V, s):
    return np.stack([V[:, 0] * (1 + 0.2 * s), 0.15 * s * np.sin(3 * V[:, 0]) * np.cos(2 * V[:, 2]) + 0.1 * s * V[:, 0], V[:, 2] - 0.05 * s * V[:, 0] ** 2], 1)


def test_open_mesh_updates(pkg):
    """set_vertices with the creation vertices: the same closest points bitwise; a deformed grid equals a grid freshly created from the
    deformed vertices in proj and decision bitwise (the shell rule reads the face normal only, which both compute alike); a flipped
    open mesh (negative "volume") is accepted; non-finite and zero-area inputs are refused, the mesh left as it was"""
    V, F = _grid()
    r = R_SHELL
    m = pkg.Mesh(V, F, r)
    P = np.concatenate([_points(V, r, 31), _near_surface(V, F, r, 32), V, V + [0, 0.03125, 0]])
    a0, q0 = m.closest(P), m.query(P)
    m.set_vertices(V)
    a1, q1 = m.closest(P), m.query(P)
    for k in a0:
        assert np.array_equal(a0[k], a1[k]), k
    assert np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
    for s in (0.5, 1.0, -0.7):
        W_ = _bend(V, s)
        m.set_vertices(W_)
        fresh = pkg.Mesh(W_, F, r)
        Pd = np.concatenate([_points(W_, r, 33), _near_surface(W_, F, r, 34), W_])
        (pa, sa), (pb, sb) = m.query(Pd), fresh.query(Pd)
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb) and 100 <= (sa > 0).sum()
        assert m.info()["depth"] == fresh.info()["depth"]
    Vc, Fc = _cube()
    c = pkg.Mesh(Vc, Fc, r)
    c.set_vertices(Vc * [1, -1, 1])                                                 # mirrored: the enclosed volume is negative, a shell does not care
    fl = pkg.Mesh(Vc * [1, -1, 1], Fc, r)
    Pc = _points(Vc, r, 35)
    assert np.array_equal(c.query(Pc)[0], fl.query(Pc)[0])
    with pytest.raises(pkg.AdmmHipError):
        pkg.Mesh(Vc, Fc).set_vertices(Vc * [1, -1, 1])                              # ... a closed mesh does
    m.set_vertices(V)
    for bad, words in ((np.where(np.arange(len(V))[:, None] == 7, np.nan, V), ("not finite",)), (np.where(np.arange(len(V))[:, None] == 3, np.inf, V), ("not finite",)),
                       (V[:-1], ("24 vertices", "25"))):
        with pytest.raises(pkg.AdmmHipError) as e:
            m.set_vertices(bad)
        for w in words:
            assert w in str(e.value), str(e.value)
    Vz = V.copy(); Vz[F[5, 2]] = V[F[5, 0]]
    with pytest.raises(pkg.AdmmHipError) as e:
        m.set_vertices(Vz)
    assert "degenerate" in str(e.value)
    a2 = m.closest(P)
    for k in a0:
        assert np.array_equal(a0[k], a2[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 5: closed meshes keep their bits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_closed_mesh_query_is_the_parents(pkg):
    """admm_hip_mesh_query on the cube, the torus and the icosphere: bitwise the arrays recorded with the library as it was before open
    surfaces existed (tests/golden/closed_mesh_query_parent.npz: 600 of test_collision_mesh's sample points each)"""
    g = golden("closed_mesh_query_parent.npz")
    t = np.array([0.25, -0.5, 1.0])
    for name in ("cube", "torus", "ico2"):
        V, F = mesh(name)
        proj, sd = pkg.mesh_query(V, F, g[name + "_pts"], t)
        assert np.array_equal(proj, g[name + "_proj"]) and np.array_equal(sd, g[name + "_sdist"]), name
        assert 50 <= (sd > 0).sum() <= 550


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 6: the context's argument checks (a host-only context)
# ---------------------------------------------------------------------------------------------------------------------------------
def _cloth(pkg, w=2, y=0.0, size=1.0):
    """a (w x w)-cell sym_plane cloth at height y: (x [n][3], tris, hinges)"""
    mg = pkg.meshgen
    x, tris = mg.sym_plane(w, w, size=size)
    x = x.copy(); x[:, 1] = y
    return x, tris, mg.bend_hinges(tris)


def test_shell_argument_checks(pkg):
    mg = pkg.meshgen
    xc, tris, _ = _cloth(pkg)
    x = np.concatenate([xc, np.random.default_rng(0).uniform(-1, 2, size=(40, 3))])
    nc = len(xc)
    s = pkg.System(device_id=-1)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TRI_STRAIN"], tris, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    Vg, Fg = _grid()
    Vc, Fc = _cube()
    og = s.add_collision_mesh(pkg.Mesh(Vg, Fg, R_SHELL), None)
    cc = s.add_collision_mesh(Vc, Fc)
    assert s.collision_mesh(og).thickness == R_SHELL and s.collision_mesh(cc).thickness == 0.0
    _expect(pkg, lambda: s.set_collision_mesh_thickness(cc, 0.1), "error 1", "mesh %d" % cc, "closed")
    for r in (0.0, -1.0, np.nan, np.inf):
        _expect(pkg, lambda: s.set_collision_mesh_thickness(og, r), "error 1", "half thickness", "positive and finite")
    _expect(pkg, lambda: s.set_collision_mesh_thickness(7, 0.1), "error 1", "mesh_id 7")
    s.set_collision_mesh_thickness(og, 0.125)
    assert s.collision_mesh(og).thickness == 0.125
    P = np.array([[0.0, 0.1, 0.0]])
    assert np.array_equal(s.collision_mesh(og).query(P)[0], [[0.0, 0.125, 0.0]])
    # sheet surfaces: node ids outside the range, a bad thickness, a non-manifold sheet; then everything a body surface refuses
    _expect(pkg, lambda: s.add_sheet_surface(0, nc - 1, tris, 0.05), "error 1", "outside [0, %d)" % (nc - 1))
    _expect(pkg, lambda: s.add_sheet_surface(1, nc, tris, 0.05), "error 1", "names node 0")
    _expect(pkg, lambda: s.add_sheet_surface(0, len(x) + 1, tris, 0.05), "error 1", "node range")
    for r in (0.0, -0.5, np.nan, np.inf):
        _expect(pkg, lambda: s.add_sheet_surface(0, nc, tris, r), "error 1", "half thickness")
    _expect(pkg, lambda: s.add_sheet_surface(0, nc, np.concatenate([tris, tris[:1]]), 0.05), "error 1", "same direction")
    sid = s.add_sheet_surface(0, nc, tris, 0.05)
    assert s.collision_mesh(sid).thickness == 0.05 and s.collision_mesh(sid).info()["n_tris"] == len(tris)
    assert s.collision_form() == 0
    floor, sheet = [0, -1, 0, 0], [0, 0, 0, sid]
    _expect(pkg, lambda: s.set_collision_shapes([FLOOR, MESH], [floor, [0, 0.1, 0, sid]]), "error 1", "shape 1", "body surface", "translation")
    s.set_collision_shapes([FLOOR, MESH], [floor, sheet])
    assert s.collision_form() == 4
    _expect(pkg, lambda: s.set_collision_friction([0.0, 0.3]), "error 1", "shape 1", "body surface")
    _expect(pkg, lambda: s.set_collision_frames([IDENT, _frame(_rot([0, 0, 1.0], 0.3), [0, 0, 0])]), "error 1", "shape 1", "body surface")
    _expect(pkg, lambda: s.update_collision_mesh(sid, xc), "error 1", "body surface")
    s.set_body_surface_friction(sid, 0.4)
    s.set_collision_mesh_thickness(sid, 0.07)
    s.set_collision_shapes([FLOOR, MESH], [floor, [0, 0, 0, cc]])
    assert s.collision_form() == 0
    s.set_collision_shapes([MESH, FLOOR], [[0.5, 0, 0, og], floor])                 # an open obstacle takes a translation
    assert s.collision_form() == 4
    s.update_collision_mesh(og, _bend(Vg, 0.5))                                      # host-only: the context's copy takes the update
    _expect(pkg, lambda: s.update_collision_mesh(og, np.where(np.arange(len(Vg))[:, None] == 2, np.nan, Vg)), "error 1", "not finite")
    assert isinstance(mg.sheet_tris(2, 2, 5), np.ndarray) and np.array_equal(mg.sheet_tris(2, 2, 5), tris + 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the shell kernel against the host routines, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
N_NODES = 65          # one full 64-lane block and one lane of a second
R_GPU = 0.125         # the half thickness of the open meshes of the kernel tests
GRID_T = np.array([0.125, -0.25, 0.0])      # the grid entry's translation in the five-entry list: exactly representable


def _kernel_meshes():
    """registered in this order: 0 the open grid, 1 the closed cube (0.6 wide), 2 the capped icosphere (open)"""
    Vc, Fc = _cube()
    return [(*_grid(), R_GPU), (0.6 * Vc, Fc, None), (*_capped_icosphere(), R_GPU)]


def _ico_vel(V):
    return np.stack([0.6 * np.sin(3 * V[:, 1]) + 0.4 * V[:, 2], -0.5 * V[:, 0] * V[:, 2] + 0.2, 0.7 * np.cos(2 * V[:, 0])], 1)      # not rigid


def _shell_lists():
    """entries (type, params, frame, mu, motion): the five-entry list -- floor, open grid, closed cube, box, capped icosphere under a
    frame, a rigid motion on the grid's entry -- and 64 translated copies of them (the frames' pivots move along)"""
    rng = np.random.default_rng(51)
    z9 = np.zeros(9)
    c_box = np.array([0.3, 0.35, -0.25])
    t_ico = np.array([-0.2, 0.15, 0.1])
    short = [(FLOOR, [0.0, -0.42, 0.0, 0.0], IDENT.copy(), 0.3, z9),
             (MESH, [*GRID_T, 0.0], IDENT.copy(), 0.5, np.array([0.4, 0.2, -0.3, 1.0, 2.0, -1.5, 0.5, 0.2, 0.1])),
             (MESH, [-0.3, 0.25, 0.3, 1.0], IDENT.copy(), 0.0, z9),
             (BOX, [0.4, 0.3, 0.4, 0.0], _frame(_rot([0.2, 0.1, 1.0], 0.6), c_box), np.inf, z9),
             (MESH, [*t_ico, 2.0], _frame(_rot(rng.normal(size=3), 0.9), t_ico + [0.05, -0.1, 0.0]), 0.7, z9)]
    full = []
    for k in range(64):
        ty, par, f, mu, mo = short[k % 5]
        d = rng.uniform(-0.25, 0.25, 3)
        par, f = list(par), f.copy()
        if ty == FLOOR:
            par[1] += 0.1 * d[1]
        elif ty == BOX:
            f[9:] += d
        else:
            par[:3] = np.asarray(par[:3]) + d
            f[9:] += d
        if ty == MESH and par[3] == 2.0 and k % 4 == 3:                             # one capped icosphere in four without a frame
            f = IDENT.copy()
        full.append((ty, par, f, [0.3, 0.0, 0.7, np.inf, 0.15][k % 5] if k >= 5 else mu, mo))
    return {"short": short, "full": full}


def _shell_case():
    """65 candidates p = dx + u within about 0.8 of the origin, a third of them within 1.5 r of the grid's plane; the first ten placed
    exactly (u = 0): on the faces of the grid's inflated box, at d2 == r^2 above and below the sheet, and on the surface (d == 0:
    a face, an edge, a vertex)"""
    dx, x0, u = _kernel_case(N_NODES, 5)
    dx, x0, u = 0.6 * dx, 0.6 * x0, 0.6 * u
    rng = np.random.default_rng(52)
    k = np.arange(10, 32)
    dx[k, 1] = GRID_T[1] + rng.uniform(-1.5 * R_GPU, 1.5 * R_GPU, len(k)) - u[k, 1]
    dx[k, 0] = rng.uniform(-0.5, 0.7, len(k)) - u[k, 0]
    r = R_GPU
    special = np.array([[0.5 + r, 0.0, 0.125], [-0.5 - r, 0.03125, -0.25], [0.25, 0.0625, 0.5 + r], [0.125, r, 0.25], [-0.25, -r, 0.125],
                        [0.0625, 0.0, 0.03125], [0.125, 0.0, 0.0], [0.25, 0.0, -0.25], [0.3125, 0.5 * r, 0.0625], [-0.375, -0.25 * r, 0.4375]]) + GRID_T
    dx[:10] = special; u[:10] = 0.0
    x0[:10] = special + 0.03 * rng.normal(size=(10, 3))
    return dx, x0, u


def _shell_compose(pkg, entries, p, x0, friction, moving):
    """the list's entries in order on the host: shape_query or Mesh.query (framed), then the friction rule on the world-space points ->
    (z, pushes per entry type / mesh, friction modes at pushes)"""
    specs = _kernel_meshes()
    meshes = [pkg.Mesh(V, F, r) for V, F, r in specs]
    pushes, modes = {}, []
    for ty, par, f, mu, motion in entries:
        vi = None
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            key = ty
        else:
            mi = int(par[3])
            key = "mesh%d" % mi
            proj, sd = meshes[mi].query(p, par[:3], frame=f)
            moved = (proj != p).any(1) if specs[mi][2] else sd > 0
            if specs[mi][2]:
                assert np.array_equal(proj[~moved], p[~moved]) and (sd[moved] >= 0).all()
            q = np.where(moved[:, None], proj, p)
            if moving and mi == 2:                                                  # the icosphere's vertex velocities at the hit, turned by R
                framed = not np.array_equal(f[:9], IDENT[:9])
                loc = _to_local(f, p) if framed else p
                vi, _, _ = pkg.mesh_velocity_query(meshes[mi], None, loc, _ico_vel(specs[2][0]), par[:3])
                if framed:
                    vi = _rotate(f, vi)
        pushes[key] = pushes.get(key, 0) + int(moved.sum())
        if friction:
            w = _np_rigid(motion if moving else np.zeros(9), q)
            if vi is not None:
                w = w + DT * vi
            q2, mode = (pkg.friction_query_moving(p, q, x0, w, mu) if moving else pkg.friction_query(p, q, x0, mu))
            modes.append(mode[moved])
            q = q2
        p = q
    return p, pushes, (np.concatenate(modes) if modes else np.zeros(0, np.int32))


def _shell_system(pkg, entries, x0, friction, moving, thickness=None):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    n = len(x0)
    s.add_nodes(x0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    for V, F, r in _kernel_meshes():
        s.add_collision_mesh(pkg.Mesh(V, F, r if r is None or thickness is None else thickness), None)
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    s.set_collision_friction([e[3] if friction else 0.0 for e in entries])
    s.initialize()
    s.set_collision_frames([e[2] for e in entries])
    if moving:
        s.set_collision_motion([e[4] for e in entries])
        s.set_collision_mesh_velocity(2, _ico_vel(_kernel_meshes()[2][0]))
    return s, b


def _shell_step(pkg, which, friction, moving):
    entries = _shell_lists()[which]
    dx, x0, u = _shell_case()
    s, b = _shell_system(pkg, entries, x0, friction, moving)
    assert s.collision_form() == 4
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    return entries, dx, x0, u, r["z"].copy(), r["u"].copy()


def test_shell_case_counts(pkg):
    """the seeds of the GPU kernel tests, checked on the host: in both lists every kind of entry pushes some of the 65 candidates, the
    exactly placed candidates do what the rule says for them, and with friction there are contacts that stick and that slip"""
    dx, x0, u = _shell_case()
    lists = _shell_lists()
    assert len(lists["short"]) == 5 and len(lists["full"]) == 64
    for which, entries in lists.items():
        _, pushes, _ = _shell_compose(pkg, entries, dx + u, x0, False, False)
        assert all(pushes.get(k, 0) >= 3 for k in (FLOOR, BOX, "mesh0", "mesh1", "mesh2")), (which, pushes)
        for moving in (False, True):
            _, _, modes = _shell_compose(pkg, entries, dx + u, x0, True, moving)
            assert (modes == 1).sum() >= 3 and (modes == 2).sum() >= 3, (which, moving, [int((modes == k).sum()) for k in range(3)])
    p = (dx + u)[:10]
    g = pkg.Mesh(*_grid(), R_GPU)
    proj, sd = g.query(p, GRID_T)
    assert np.array_equal(proj[:5], p[:5]) and np.isneginf(sd[:5]).all()              # the box's faces, d2 == r^2: not collisions
    assert np.array_equal(sd[5:8], np.full(3, R_GPU)) and np.array_equal(proj[5:8, 1], np.full(3, GRID_T[1] + R_GPU))      # d == 0
    assert (sd[8:] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "friction", "moving"])
@pytest.mark.parametrize("which", ["short", "full"])
def test_shell_kernel_equals_host_composition(pkg, which, case):
    """65 nodes, one local step of the collision batch alone: z and u bitwise equal to the host composition of admm_hip_mesh_query_framed,
    admm_hip_shape_query, admm_hip_mesh_velocity_query and the friction queries, in list order -- without friction, with per-entry
    coefficients, and with a rigid motion on the grid's entry and vertex velocities on the icosphere"""
    friction, moving = case != "plain", case == "moving"
    entries, dx, x0, u, z, un = _shell_step(pkg, which, friction, moving)
    want, pushes, modes = _shell_compose(pkg, entries, dx + u, x0, friction, moving)
    print("%s list, %s: pushes %s, none / stick / slip %s" % (which, case, pushes, [int((modes == k).sum()) for k in range(3)]))
    assert np.array_equal(z, want), (np.abs(z - want).max(), np.flatnonzero((z != want).any(1)))
    assert np.array_equal(un, u + (dx - want))
    if moving:
        still, _, _ = _shell_compose(pkg, entries, dx + u, x0, True, False)
        assert np.abs(still - want).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 2: a list without an open mesh launches what it launched; GPU 3: the thickness under a captured graph
# ---------------------------------------------------------------------------------------------------------------------------------
def _drop_scene(n=N_NODES, seed=61):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (n, 3))
    x[:, 1] = rng.uniform(0.35, 0.6, n)
    return x


def _drop_system(pkg, x, with_sheet, thickness=R_GPU):
    Vc, Fc = _cube()
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    s.cube = s.add_collision_mesh(0.6 * Vc, Fc)
    if with_sheet:
        s.sheet = s.add_collision_mesh(pkg.Mesh(*_grid(), thickness), None)
    s.base = ([FLOOR, MESH], [[0, -0.2, 0, 0], [0, 0.0, 0, s.cube]])
    s.set_collision_shapes(*s.base)
    s.initialize()
    return s


def _run(s, frames, iters=10):
    out = []
    for _ in range(frames):
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


def _same_frames(a, b):
    return len(a) == len(b) and all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a, b))


@pytest.mark.gpu
def test_no_open_mesh_no_change(pkg):
    """65 particles dropped on a floor and a closed cube.  A context with an open mesh registered but not named: the frames, the
    collision_form and the graph state of the same context without it.  Naming the sheet (far away, so that nothing touches it)
    changes the form to 4 and drops the graphs once; the shell kernel's code for closed meshes and analytic entries gives the other
    kernels' bits; taking the sheet out of the list returns to the previous form, dropping the graphs once more"""
    x = _drop_scene()
    a, b = _drop_system(pkg, x, False), _drop_system(pkg, x, True)
    assert a.collision_form() == b.collision_form() == 0
    ra, rb = _run(a, 4), _run(b, 4)
    assert _same_frames(ra, rb)
    assert a.graph_state() == b.graph_state() and a.graph_state()["frame_graph_iters"] == 10, (a.graph_state(), b.graph_state())
    far = (b.base[0] + [MESH], b.base[1] + [[50.0, 0, 0, b.sheet]])
    b.set_collision_shapes(*far)
    assert b.collision_form() == 4
    g = b.graph_state()
    assert not g["iter_graph"] and g["frame_graph_iters"] == 0, g                      # dropped
    ra, rb = _run(a, 2), _run(b, 2)
    assert _same_frames(ra, rb)
    assert b.graph_state()["frame_graph_iters"] == 10
    b.set_collision_shapes(*far)                                                     # the same form: the graphs stay
    assert b.graph_state()["frame_graph_iters"] == 10
    ra, rb = _run(a, 2), _run(b, 2)
    assert _same_frames(ra, rb)
    b.set_collision_shapes(*b.base)
    assert b.collision_form() == 0 and b.graph_state()["frame_graph_iters"] == 0
    ra, rb = _run(a, 3), _run(b, 3)
    assert _same_frames(ra, rb)
    assert a.graph_state()["frame_graph_iters"] == b.graph_state()["frame_graph_iters"] == 10
    free_y = x[:, 1] - DT * DT * G * 11 * 12 / 2                                       # eleven frames of free fall
    assert np.abs(rb[-1][0].reshape(-1, 3)[:, 1] - free_y).max() > 1e-2               # some particles met the cube


def _sheet_drop(pkg, x, r0, change_to=None, frames=14):
    """the drop scene with the sheet at y = 0.25 in the list; -> (frames, graph state at the end, graph state right after the call)"""
    s = _drop_system(pkg, x, True, thickness=r0)
    s.set_collision_shapes(s.base[0] + [MESH], s.base[1] + [[0, 0.25, 0, s.sheet]])
    out, after = [], None
    for f in range(frames):
        if change_to is not None and f == 3:
            s.set_collision_mesh_thickness(s.sheet, change_to)
            after = s.graph_state()
        s.step(10)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out, s.graph_state(), after


@pytest.mark.gpu
def test_thickness_under_a_captured_graph(pkg):
    """set_collision_mesh_thickness between frames 3 and 4 in graph mode: from there on bitwise the frames of a context that had the new
    value from the start and the same first three frames... which it cannot have -- so: the first three frames do not touch the sheet
    (the particles are still above it with either value), and the whole run equals the fresh context's; no re-capture happens"""
    x = _drop_scene()
    x[:, 1] += 0.25
    fresh, g0, _ = _sheet_drop(pkg, x, 0.1875)
    thin, _, _ = _sheet_drop(pkg, x, 0.0625)
    changed, g1, after = _sheet_drop(pkg, x, 0.0625, change_to=0.1875)
    assert _same_frames(fresh[:3], thin[:3]) and not _same_frames(fresh, thin)        # untouched for three frames, then the value matters
    assert _same_frames(changed, fresh)
    assert after["frame_graph_iters"] == 10 and after["iter_graph"], after            # the call left the captured graphs alone
    assert g1 == g0 and g1["frame_graph_iters"] == 10, (g0, g1)                       # ... and the same number of graph launches followed


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 4: launch modes; GPU 5: device updates
# ---------------------------------------------------------------------------------------------------------------------------------
def _mode_results(pkg):
    out = {}
    for which in ("short", "full"):
        _, _, _, _, z, un = _shell_step(pkg, which, True, True)
        out["z_" + which], out["u_" + which] = z, un
    x = _drop_scene()
    x[:, 1] += 0.25
    fr, _, _ = _sheet_drop(pkg, x, 0.125)
    out["drop_x"] = np.array([f[0] for f in fr]); out["drop_v"] = np.array([f[1] for f in fr])
    return out


def _child_main(path):
    from __graft_entry__ import load_package
    np.savez(path, **_mode_results(load_package()))


@pytest.mark.gpu
def test_shell_launch_modes_bitwise(pkg, monkeypatch, tmp_path):
    """eager, iteration graph, frame graph in this process, and ADMM_HIP_LOCAL_MULTI=0 in a fresh child process: the kernel scenes and
    14 frames of particles dropped on a sheet, a cube and a floor give the same bits"""
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
    code = "import sys; sys.path[:0] = [%r, %r]; import test_collision_shell as t; t._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.load(path)
    for name, v in res[keys[0]].items():
        assert np.array_equal(got[name], v), name
    d = res[keys[0]]["drop_x"].reshape(14, -1, 3)
    assert np.abs(d[-1] - d[0]).max() > 1e-2


@pytest.mark.gpu
def test_device_update_follows_the_host_object(pkg):
    """three admm_hip_update_collision_mesh calls on the open grid: after each the device's projection of 65 + 600 points equals the
    host object's under admm_hip_mesh_set_vertices bit for bit; a refused update (a NaN vertex) leaves the live sheet intact"""
    V, F = _grid()
    r = R_GPU
    t = np.array([0.1, 0.2, -0.3])
    P = np.ascontiguousarray(np.concatenate([_points(_bend(V, 1.0), r, 71, 400), _near_surface(V, F, r, 72, 265)]) + t)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(P.ravel(), np.ones(P.size))
    b = s.add_forces(KIND["COLLISION"], np.arange(len(P), dtype=np.int32), [W])
    mid = s.add_collision_mesh(pkg.Mesh(V, F, r), None)
    s.set_collision_shapes([MESH], [[*t, mid]])
    s.initialize()
    host = pkg.Mesh(V, F, r)

    def device():
        s.write_local(b, u=np.zeros_like(P))
        s.local_step_dx(b, P)
        return s.read_local(b)["z"]
    assert np.array_equal(device(), host.query(P, t)[0])
    for k, sc in enumerate((0.5, 1.0, -0.7)):
        Wd = _bend(V, sc)
        s.update_collision_mesh(mid, Wd)
        host.set_vertices(Wd)
        want = host.query(P, t)[0]
        z = device()
        assert np.array_equal(z, want), (k, np.abs(z - want).max())
        assert 30 <= (want != P).any(1).sum() <= len(P) - 30
        if k == 1:
            bad = Wd.copy(); bad[11, 2] = np.nan
            with pytest.raises(pkg.AdmmHipError) as e:
                s.update_collision_mesh(mid, bad)
            assert "not finite" in str(e.value)
            assert np.array_equal(device(), want)
    s.update_collision_mesh(mid, V * [1, 1, -1])                                     # mirrored (every normal flipped): no volume condition on a sheet
    host.set_vertices(V * [1, 1, -1])
    assert np.array_equal(device(), host.query(P, t)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 6: free particles on a flat sheet against a floor
# ---------------------------------------------------------------------------------------------------------------------------------
def _particle_run(pkg, x, types, params, meshes, frames=20, iters=20):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    for m in meshes:
        s.add_collision_mesh(m, None)
    s.set_collision_shapes(types, params)
    s.initialize()
    xs, vs = [], []
    for _ in range(frames):
        s.step(iters)
        xs.append(s.m_x.reshape(-1, 3).copy()); vs.append(s.m_v.reshape(-1, 3).copy())
    return np.array(xs), np.array(vs)


@pytest.mark.gpu
def test_free_particles_on_a_flat_sheet(pkg):
    """130 free particles fall from up to 0.15 above the surface of the flat 4 x 4 grid at y = 0 with r = 0.125, 20 frames x 20
    iterations at dt = 0.02.  The 90 over the sheet's interior follow, to 1e-9 (the project's bound for collision trajectories), the
    same particles over a floor at y = r; the 40 more than r outside its outline are bitwise those of a control whose list holds only
    a far-away floor.  From 0.15 the speed at contact is sqrt(2 g 0.15) = 1.71, so no particle moves more than 0.035 < r / 2 a frame
    near the sheet: asserted from the floor run's velocities.  (The rule has no side memory: a faster particle would cross the
    mid-surface and leave below.)  Measured on the MI355X: interior |x - floor| 1.05e-15, |v - floor| 7.29e-15, largest travel per frame
    0.0314."""
    r = 0.125
    rng = np.random.default_rng(81)
    n, nin = 130, 90
    x = np.zeros((n, 3))
    x[:nin, 0] = rng.uniform(-0.4, 0.4, nin); x[:nin, 2] = rng.uniform(-0.4, 0.4, nin)
    side = rng.uniform(size=n - nin) < 0.5
    far = rng.uniform(0.5 + 1.5 * r, 0.9, n - nin) * np.where(rng.uniform(size=n - nin) < 0.5, -1, 1)
    near = rng.uniform(-0.9, 0.9, n - nin)
    x[nin:, 0] = np.where(side, far, near); x[nin:, 2] = np.where(side, near, far)
    x[:, 1] = r + rng.uniform(0.0, 0.15, n)
    sheet = pkg.Mesh(*_grid(), r)
    xs, vs = _particle_run(pkg, x, [MESH], [[0, 0, 0, 0]], [sheet])
    xf, vf = _particle_run(pkg, x, [FLOOR], [[0, r, 0, 0]], [])
    xc, vc = _particle_run(pkg, x, [FLOOR], [[0, -100.0, 0, 0]], [])
    travel = np.abs(vf[:, :nin, 1]).max() * DT
    assert travel <= r / 2, travel
    ex, ev = np.abs(xs[:, :nin] - xf[:, :nin]).max(), np.abs(vs[:, :nin] - vf[:, :nin]).max()
    print("flat sheet: interior |x - floor| %.3g, |v - floor| %.3g; largest travel per frame %.4f (r / 2 = %.4f)" % (ex, ev, travel, r / 2))
    assert ex <= 1e-9 and ev <= 1e-9, (ex, ev)
    assert np.abs(xf[-1, :nin, 1] - r).max() < 1e-3 and (xs[-1, :nin, 1] > r - 1e-3).all()      # they rest on the shell's upper face
    assert np.array_equal(xs[:, nin:], xc[:, nin:]) and np.array_equal(vs[:, nin:], vc[:, nin:])
    assert xc[-1, nin:, 1].max() < -0.5                                               # ... and those fell on


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 7: a sheet surface follows its cloth
# ---------------------------------------------------------------------------------------------------------------------------------
R_CLOTH = 0.125
NC = 25               # the cloth: the 5 x 5 nodes of the 4 x 4 grid, corners anchored


def _cloth_scene(seed=91, n_part=N_NODES):
    """-> (x, m, tris, corners): the cloth's nodes first, then 65 free particles up to 0.1 above the shell over and around it"""
    V, F = _grid()
    rng = np.random.default_rng(seed)
    P = np.zeros((n_part, 3))
    P[:, 0] = rng.uniform(-0.65, 0.65, n_part); P[:, 2] = rng.uniform(-0.65, 0.65, n_part)
    P[:, 1] = R_CLOTH + rng.uniform(0.0, 0.1, n_part)
    x = np.concatenate([V, P])
    m = np.concatenate([np.full(NC, 0.02), np.full(n_part, 1.0)])
    return x, m, F, np.array([0, 4, 20, 24], dtype=np.int32)


def _cloth_system(pkg, route, rank=0, world=1, mode=None, mu=0.0, v0=None):
    """route "sheet": add_sheet_surface; "obstacle": the same open mesh as an obstacle owned by the cloth's nodes, updated by the caller"""
    x, m, F, corners = _cloth_scene()
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TRI_STRAIN"], F, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["BEND"], pkg.meshgen.bend_hinges(F), [20.0])
    s.add_forces(KIND["ANCHOR"], corners, [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    if world > 1:
        s.set_shard(rank, world)
        if mode:
            s.set_shard_mode(mode)
    if route == "sheet":
        s.mid = s.add_sheet_surface(0, NC, F, R_CLOTH)
        if mu:
            s.set_body_surface_friction(s.mid, mu)
    else:
        s.mid = s.add_collision_mesh(pkg.Mesh(x[:NC], F, R_CLOTH), None)
        s.set_collision_mesh_owner(s.mid, 0, NC)
    s.set_collision_shapes([MESH], [[0, 0, 0, s.mid]])
    s.route = route
    return s


def _cloth_frames(s, frames=5, iters=10):
    out = []
    for f in range(frames):
        if s.route == "obstacle":
            s.update_collision_mesh(s.mid, s.m_x.reshape(-1, 3)[:NC])
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


@pytest.mark.gpu
def test_sheet_surface_follows_its_nodes_launch_modes(pkg, monkeypatch):
    """a 5 x 5-node cloth (LimitedTriangleStrain + BendForce, corners anchored) sagging under gravity and 65 particles falling on its
    shell: five frames through add_sheet_surface are bitwise the host-driven route (an obstacle copy given x[cloth nodes] before every
    step), in every launch mode; the status counts five updates; the cloth's own nodes, which carry collision elements that list the
    sheet, move exactly as in a control whose list holds a far-away floor"""
    res = {}
    for env in ({}, {"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}, {"ADMM_HIP_LOCAL_MULTI": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        a = _cloth_system(pkg, "sheet"); a.initialize()
        o = _cloth_system(pkg, "obstacle"); o.initialize()
        assert a.collision_form() == 4
        ra, ro = _cloth_frames(a), _cloth_frames(o)
        assert _same_frames(ra, ro), env
        assert a.body_surface_status(a.mid) == dict(updated=5, refused=0, last_bad_tri=-1)
        res[tuple(env.items())] = ra
    keys = list(res)
    for k in keys[1:]:
        assert _same_frames(res[keys[0]], res[k]), k
    for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
        monkeypatch.delenv(k, raising=False)
    c = _cloth_system(pkg, "obstacle")
    c.set_collision_shapes([FLOOR], [[0, -100.0, 0, 0]])
    c.initialize()
    c.route = "control"
    rc = _cloth_frames(c)
    X = np.array([f[0].reshape(-1, 3) for f in res[keys[0]]]); Xc = np.array([f[0].reshape(-1, 3) for f in rc])
    assert np.array_equal(X[:, :NC], Xc[:, :NC])                                     # the cloth's own nodes skip their sheet
    assert np.abs(X[-1, :NC, 1]).max() > 1e-3                                        # ... while it sags
    assert np.abs(X[:, NC:] - Xc[:, NC:]).max() > 1e-2                                # and the particles are held


@pytest.mark.gpu
def test_sheet_surface_refused_frame(pkg):
    """a NaN written into cloth node 12 before the third frame: the step returns ADMM_OK, the frame is counted as refused with the
    lowest triangle of that node named, and the last good surface (the cloth as the second frame found it) is still the one the
    collision kernel reads: a local step on finite candidates equals the host query on that surface.  With x and v restored the
    next frame's update is applied again."""
    a = _cloth_system(pkg, "sheet"); a.initialize()
    F = _grid()[1]
    a.step(10)
    good = a.m_x.reshape(-1, 3)[:NC].copy()                                          # what the second frame's update reads
    a.step(10)
    X, V = a.m_x.copy(), a.m_v.copy()
    bad = X.reshape(-1, 3).copy(); bad[12, 1] = np.nan
    a.m_x = bad.ravel()
    a.step(10)                                                                       # no exception: ADMM_OK
    st = a.body_surface_status(a.mid)
    assert st == dict(updated=2, refused=1, last_bad_tri=int(np.flatnonzero((F == 12).any(1))[0])), st
    n = len(X) // 3
    P = np.concatenate([good, _near_surface(good, F, R_CLOTH, 93, n - NC)])
    b = 3                                                                            # the collision batch
    a.write_local(b, u=np.zeros((n, 3)))
    a.local_step_dx(b, P)
    z = a.read_local(b)["z"]
    want = pkg.Mesh(good, F, R_CLOTH).query(P)[0]
    assert np.array_equal(z[NC:], want[NC:]) and 10 <= (want[NC:] != P[NC:]).any(1).sum()
    assert np.array_equal(z[:NC], P[:NC])                                            # the owner's nodes skip it
    a.m_x = X; a.m_v = V
    a.step(10)
    assert a.body_surface_status(a.mid) == dict(updated=3, refused=1, last_bad_tri=st["last_bad_tri"])      # (the duals keep the NaN: only the surface is looked at)


@pytest.mark.gpu
def test_sheet_surface_two_subtree_shards(pkg, monkeypatch):
    """the same five frames in two subtree shards: the ranks bitwise equal, both routes bitwise equal, and within 1e-9 of one rank"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    ref = _cloth_system(pkg, "sheet"); ref.initialize()
    refx = _cloth_frames(ref)
    out = {}
    for route in ("sheet", "obstacle"):
        shards = [_cloth_system(pkg, route, rank=r, world=2, mode="subtree") for r in range(2)]
        hooks = _thread_allreduce_hooks(2)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(shards)
        res, errs = [None, None], []

        def run(r):
            try:
                res[r] = _cloth_frames(shards[r])
            except Exception as e:  # noqa: BLE001
                errs.append((r, e))
        th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join(timeout=300)
        assert not errs, errs
        assert _same_frames(res[0], res[1]), route
        out[route] = res[0]
    assert _same_frames(out["sheet"], out["obstacle"])
    for f in range(5):
        d = np.abs(out["sheet"][f][0] - refx[f][0]).max()
        assert d < 1e-9, (f, d)


def test_cpp_shell_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_shell", pkg))


@pytest.mark.gpu
def test_class_api_collision_sheet(pkg, tmp_path):
    """the cloth scene through admm::System with a CollisionSheet in the CollisionForce's list: bitwise the C ABI's frames"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_shell", pkg)
    x, m, F, corners = _cloth_scene()
    hinges = pkg.meshgen.bend_hinges(F)
    frames, iters = 5, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(F), len(hinges), len(corners), NC], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (F, hinges, corners):
            np.asarray(a).astype(np.int32).tofile(f)
        np.array([R_CLOTH, DT, 0.0]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(outp).reshape(frames, 2, len(x) * 3)
    s = _cloth_system(pkg, "sheet"); s.initialize()
    want = _cloth_frames(s, frames, iters)
    for f in range(frames):
        assert np.array_equal(got[f, 0], want[f][0]) and np.array_equal(got[f, 1], want[f][1]), (f, np.abs(got[f, 0] - want[f][0]).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 8: contact that a control lacks; GPU 9: friction on a sheet
# ---------------------------------------------------------------------------------------------------------------------------------
def _block_over_sheet(pkg, listed, frames=10, iters=20):
    """a 2 x 2 x 2-cell tet block, scaled to 0.3 wide, r + 0.01 above a fully anchored 5 x 5-node cloth at y = 0"""
    mg = pkg.meshgen
    r = R_CLOTH
    V, F = _grid()
    xb, tets = mg.bar(2, 2, 2)
    xb = (xb - xb.min(0)) / (xb.max(0) - xb.min(0)).max() * 0.3
    xb = xb - [0.15, 0.0, 0.15] + [0.0, r + 0.01, 0.0]
    mb = mg.lumped_tet_mass(xb, tets, 1000.0)
    x = np.concatenate([V, xb])
    m = np.concatenate([np.full(NC, 0.02), mb])
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets + NC, [2e4])
    s.add_forces(KIND["TRI_STRAIN"], F, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["BEND"], mg.bend_hinges(F), [20.0])
    s.add_forces(KIND["ANCHOR"], np.arange(NC, dtype=np.int32), [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(NC, len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    mid = s.add_sheet_surface(0, NC, F, r)
    s.set_collision_shapes([MESH] if listed else [FLOOR], [[0, 0, 0, mid]] if listed else [[0, -100.0, 0, 0]])
    s.initialize()
    ys, vmax = [], 0.0
    for _ in range(frames):
        s.step(iters)
        ys.append(s.m_x.reshape(-1, 3)[NC:, 1].min())
        vmax = max(vmax, np.abs(s.m_v.reshape(-1, 3)[NC:, 1]).max())
    return np.array(ys), vmax, s.m_x.reshape(-1, 3)[:NC, 1].copy()


@pytest.mark.gpu
def test_block_lands_on_a_sheet_a_control_falls_through(pkg):
    """a small tet block starts r + 0.01 above a fully anchored cloth sheet (r = 0.125) and falls for ten frames of 20 iterations, its
    collision force listing the sheet: its lowest node ends above the sheet's mid-surface (y = 0); in the control, the sheet not
    listed, it ends below.  The block meets the shell within two frames at no more than 0.6 m/s, 0.012 of travel a frame, far below
    r (the rule's condition r > closing speed x dt; asserted from the contact run's velocities).  Measured on the MI355X: lowest node
    after ten frames 0.1250 with the sheet listed, -0.0806 in the control; largest |v_y| 0.582."""
    ys, vmax, cloth = _block_over_sheet(pkg, True)
    yc, _, _ = _block_over_sheet(pkg, False)
    print("block over a sheet: lowest node after ten frames %.4f (listed), %.4f (control); largest |v_y| %.3f" % (ys[-1], yc[-1], vmax))
    assert np.abs(cloth).max() < 1e-3                                                # anchored: the mid-surface stays at y = 0
    assert vmax * DT < R_CLOTH
    assert ys[-1] > cloth.max() and ys.min() > cloth.max()
    assert yc[-1] < cloth.min()


@pytest.mark.gpu
def test_friction_on_a_moving_sheet(pkg):
    """set_body_surface_friction(mu = inf) on a flat sheet whose nodes all start every frame with the velocity (0.5, 0, -0.3) (they are
    anchored, so the sheet stays in place like a conveyor belt; the caller writes v before each step): particles released at rest on
    the shell under gravity advance by v dt per frame tangentially, to 1e-12 from the seventh frame on (the conveyor check of
    test_moving_friction and its transient, on a sheet; measured on the MI355X: 1.15e-14)"""
    r = R_CLOTH
    V, F = _grid(4, 4.0)                                                            # 4 m wide: the particles stay over it
    nv = len(V)
    vb = np.array([0.5, 0.0, -0.3])
    rng = np.random.default_rng(95)
    n = N_NODES
    P = np.zeros((n, 3)); P[:, 0] = rng.uniform(-1, 1, n); P[:, 2] = rng.uniform(-1, 1, n); P[:, 1] = r
    x = np.concatenate([V, P])
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["ANCHOR"], np.arange(nv, dtype=np.int32), [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(nv, len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    mid = s.add_sheet_surface(0, nv, F, r)
    s.set_body_surface_friction(mid, np.inf)
    s.set_collision_shapes([MESH], [[0, 0, 0, mid]])
    s.initialize()
    assert s.collision_form() == 4
    frames = 12
    xs = []
    for f in range(frames):
        v = s.m_v.reshape(-1, 3).copy()
        v[:nv] = vb
        s.m_v = v.ravel()
        s.step(20)
        xs.append(s.m_x.reshape(-1, 3).copy())
    adv = np.diff(np.array(xs), axis=0)[:, nv:]
    err = np.abs(adv[6:][:, :, [0, 2]] - DT * vb[[0, 2]]).max()
    print("friction on a sheet: tangential advance per frame against v dt from frame 7 on, max error %.3g" % err)
    assert err <= 1e-12, err
    assert np.abs(xs[-1][:nv] - V).max() < 0.05                                       # the belt stayed
    assert s.body_surface_status(mid)["updated"] == frames
