"""Oriented collision obstacles (admm_hip_set_collision_frames, ADMM_SHAPE_BOX): the host evaluations admm_hip_shape_query and
admm_hip_mesh_query_framed against extended-precision numpy restatements, the box rule case by case, the argument checks, and on the
GPU: the framed form of the collision kernel bit for bit against a composition of the host routines (without friction, with friction,
with moving friction), identity frames as the existing path, the per-batch launch path in a child process, and a block on a ramp
against the same block on a level floor under turned gravity.

No reference counterpart: the expected values come from numpy in here."""

import os
import subprocess
import sys

import numpy as np
import pytest

from checkers import KIND
from test_collision_friction import CYLINDER, DT, G, W, _bar, _bar_frames, _expect, _kernel_case, _np_cylinder, _points_system, _same
from test_collision_mesh import FLOOR, MESH, SPHERE, _closest_on_tris, _np_floor, _np_sphere, mesh, orient
from test_moving_friction import _np_rigid

BOX = 4
EPS = np.finfo(np.float64).eps
L = np.longdouble
IDENT = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# rotations, the two maps and the rules in numpy (any float type)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    """Rodrigues' formula in float64; axis need not be normalised"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _quarter(axis, turns):
    """an exact turn by `turns` x 90 degrees about a coordinate axis: entries 0 and +-1 only"""
    return np.round(_rot(np.eye(3)[axis], turns * np.pi / 2))


def _frame(R, o):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(o, dtype=np.float64).reshape(3)])


def _to_local(f, p):
    """q_j = o_j + (R_0j e_0 + (R_1j e_1 + R_2j e_2)), e = p - o: the order include/admm_hip.h documents; the dtype of p decides"""
    f = np.asarray(f, dtype=p.dtype)
    R, o = f[:9].reshape(3, 3), f[9:]
    e = p - o
    return np.stack([o[j] + (R[0, j] * e[:, 0] + (R[1, j] * e[:, 1] + R[2, j] * e[:, 2])) for j in range(3)], 1)


def _to_world(f, q):
    f = np.asarray(f, dtype=q.dtype)
    R, o = f[:9].reshape(3, 3), f[9:]
    e = q - o
    return np.stack([o[j] + (R[j, 0] * e[:, 0] + (R[j, 1] * e[:, 1] + R[j, 2] * e[:, 2])) for j in range(3)], 1)


def _rotate(f, v):
    R = np.asarray(f, dtype=v.dtype)[:9].reshape(3, 3)
    return np.stack([R[j, 0] * v[:, 0] + (R[j, 1] * v[:, 1] + R[j, 2] * v[:, 2]) for j in range(3)], 1)


def _np_rule(ty, par, c, q):
    """the unframed rule of one analytic entry on local points q (any float type) -> (q', moved, margin): margin = how far the decision
    is from flipping (the penetration depth's size; for a box that is pushed also the gap between its two smallest depths)"""
    par = np.asarray(par, dtype=q.dtype)
    out = q.copy()
    if ty == FLOOR:
        dep = par[1] - q[:, 1]
        hit = dep > 0
        out[hit, 1] = par[1]
        return out, hit, np.abs(dep)
    if ty in (SPHERE, CYLINDER):
        d = q - par[:3]
        if ty == CYLINDER:
            d[:, 2] = 0
        nrm = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
        dep = par[3] - nrm
        hit = dep > 0
        for j in range(3 if ty == SPHERE else 2):
            out[hit, j] = par[j] + par[3] * (d[hit, j] / nrm[hit])
        return out, hit, np.abs(dep)
    assert ty == BOX
    c = np.asarray(c, dtype=q.dtype)
    d = q - c
    g = par[:3] - np.abs(d)
    hit = (g > 0).all(1)
    ax = np.argmin(g, axis=1)                                                       # (the first of equal minima: the lowest axis)
    rows = np.nonzero(hit)[0]
    out[rows, ax[rows]] = np.where(d[rows, ax[rows]] >= 0, c[ax[rows]] + par[ax[rows]], c[ax[rows]] - par[ax[rows]])
    gs = np.sort(g, axis=1)
    return out, hit, np.where(hit, np.minimum(gs[:, 0], gs[:, 1] - gs[:, 0]), np.abs(g.min(1)))


def _np_entry(ty, par, f, p):
    """one entry with its frame, restated: to local coordinates, the rule, and back for the points it moved -> (out, moved, margin, q')"""
    f = np.asarray(f, dtype=p.dtype)
    q = _to_local(f, p)
    q2, hit, margin = _np_rule(ty, par, f[9:], q)
    return np.where(hit[:, None], _to_world(f, q2), p), hit, margin, q2


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: admm_hip_shape_query against the longdouble restatement
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = {FLOOR: [0.0, -0.3, 0.0, 0.0], SPHERE: [0.3, -0.2, 0.4, 0.6], CYLINDER: [-0.2, 0.3, 0.0, 0.5], BOX: [0.4, 0.25, 0.6, 0.0]}


def _rotations():
    rng = np.random.default_rng(21)
    out = [("random %d" % k, _rot(rng.normal(size=3), rng.uniform(0.2, 3.0))) for k in range(4)]
    out += [("quarter turn about axis %d" % a, _quarter(a, 1)) for a in range(3)]
    out += [("half turn about axis %d" % a, _quarter(a, 2)) for a in range(3)]
    return out


def _local_points(ty, par, c, n, rng, scale):
    """n local points for the entry, half of them inside: the penetration depth (and a box's gap between its two smallest depths) at
    least 0.01 * max(1, 1e-3 * scale) away from zero -- above 1e-6 of the scale for every scale used here"""
    m = 0.01 * max(1.0, 1e-3 * scale)
    inside = rng.uniform(size=n) < 0.5
    par = np.asarray(par)
    if ty == FLOOR:
        q = rng.uniform(-1, 1, (n, 3))
        q[:, 1] = par[1] + np.where(inside, -1, 1) * rng.uniform(m, 0.5 + m, n)
        return q
    if ty in (SPHERE, CYLINDER):
        d = rng.normal(size=(n, 3))
        if ty == CYLINDER:
            d[:, 2] = 0
        d /= np.linalg.norm(d, axis=1)[:, None]
        r = par[3] * np.where(inside, rng.uniform(0.4, 0.9, n), rng.uniform(1.1, 1.6, n))      # depth in [0.1 R, 0.6 R]: the push stretches an error by R / r <= 2.5
        q = par[:3] + r[:, None] * d
        if ty == CYLINDER:
            q[:, 2] = rng.uniform(-1, 1, n)
        return q
    h = par[:3]
    g = np.empty((n, 3))
    for i in range(n):
        ax = rng.permutation(3)
        g0 = rng.uniform(2 * m, 0.3 * h.min())
        g[i, ax[0]] = g0 if inside[i] else -rng.uniform(2 * m, 0.2)
        g[i, ax[1]] = rng.uniform(g0 + 2 * m, 0.9 * h[ax[1]]) if h[ax[1]] * 0.9 > g0 + 2 * m else g0 + 2 * m
        g[i, ax[2]] = rng.uniform(g0 + 2 * m, 0.9 * h[ax[2]]) if h[ax[2]] * 0.9 > g0 + 2 * m else g0 + 2 * m
    sgn = np.where(rng.uniform(size=(n, 3)) < 0.5, -1.0, 1.0)
    return np.asarray(c) + sgn * (h - g)


def _shape_query_cases():
    rng = np.random.default_rng(22)
    for name, R in _rotations():
        for far in (False, True):
            for ty, par in SHAPES.items():
                o = rng.uniform(-0.5, 0.5, 3) if not far else 1e3 * _rot(rng.normal(size=3), 1.0)[0]      # |o| = 1e3
                f = _frame(R, o)
                scale = max(1.0, np.linalg.norm(o))
                par = list(par)
                if ty == BOX and far:                                               # (half extents the far scale's margin fits into)
                    par = [4.0, 2.5, 6.0, 0.0]
                q = _local_points(ty, par, o, 40, rng, scale)
                p = _to_world(f.astype(L), q.astype(L)).astype(np.float64)
                yield "%s, %s pivot, type %d" % (name, "far" if far else "near", ty), ty, par, f, p, scale


def test_shape_query_vs_longdouble(pkg):
    """Floor, sphere, z-cylinder and box under 4 random rotations, the quarter and half turns about every axis, each with a pivot near
    the shape and one at |o| = 1e3: 40 points per case, half inside, built in local coordinates so that the penetration depth (and the
    box's gap between its two smallest depths) is at least 1e-5 of the scale from zero -- the longdouble restatement's decision is
    then beyond doubt and must be matched exactly, with no case left out.

    Tolerance, per component.  With e = p - o and e' = q' - o:  e has one rounding (eps/2 |e|), the three products and two sums of
    R^T e add at most 2 eps |e|_1 <= 4 eps |e|, and the sum with o rounds by eps/2 |q_j| <= eps/2 (|o_j| + |e|): the local point is off
    by at most 5 eps |e| + eps/2 |o|.  The rule passes that on stretched by at most R / r <= 2.5 (sphere and cylinder, by the choice of
    depths; 1 for floor and box) and adds its own rounding, at most 4 eps of the size of q', which is <= |o| + |e'|.  The way back does
    the same three steps on e' and keeps the incoming error's size (R is orthogonal to 1e-12).  In all: below
    (12.5 |e| + 9 |e'|) eps + 6 eps |o|  <=  16 eps (|p - o| + |q' - o|) + 8 eps |o|.  The |o| term is the spacing of doubles at the
    size of q and p' themselves (both are sums with o); where the pivot is far from the shape it is of the size of |p - o| anyway."""
    worst = 0.0
    n_cases = 0
    for name, ty, par, f, p, scale in _shape_query_cases():
        want, hit, margin, q2 = _np_entry(ty, par, f.astype(L), p.astype(L))
        assert (margin >= 1e-6 * scale).all(), (name, float(margin.min()))
        got, moved = pkg.shape_query(ty, par, p, f)
        assert np.array_equal(moved, hit), name
        assert 8 <= hit.sum() <= 32, (name, hit.sum())
        o = f[9:]
        tol = 16 * EPS * (np.linalg.norm(p - o, axis=1) + np.linalg.norm((q2 - o.astype(L)).astype(np.float64), axis=1)) + 8 * EPS * np.linalg.norm(o)
        err = np.abs((got.astype(L) - want).astype(np.float64))
        assert (err <= tol[:, None]).all(), (name, (err / tol[:, None]).max())
        assert np.array_equal(got[~hit], p[~hit]), name                              # not moved: the same bits, no round trip
        # the float64 restatement in the documented order: the same bits
        same, _, _, _ = _np_entry(ty, par, f, p)
        assert np.array_equal(got, same), name
        worst = max(worst, (err / tol[:, None]).max())
        n_cases += 1
    print("shape_query vs longdouble: %d cases, worst error / bound %.3g" % (n_cases, worst))
    assert n_cases == 10 * 2 * 4


def test_shape_query_identity_is_the_existing_rule(pkg):
    """frame NULL and the identity frame (any pivot): bitwise the float64 closed forms the existing collision tests compare the
    unframed kernels with (floor, sphere, z-cylinder)"""
    rng = np.random.default_rng(23)
    p = rng.uniform(-1, 1, (500, 3))
    want = {FLOOR: _np_floor(p, SHAPES[FLOOR][1]), SPHERE: _np_sphere(p, np.array(SHAPES[SPHERE][:3]), SHAPES[SPHERE][3]),
            CYLINDER: _np_cylinder(p, np.array(SHAPES[CYLINDER][:3]), SHAPES[CYLINDER][3])}
    for ty, w in want.items():
        for f in (None, IDENT, _frame(np.eye(3), [0.3, -7.0, 2.0])):
            got, moved = pkg.shape_query(ty, SHAPES[ty], p, f)
            assert np.array_equal(got, w), ty
            assert np.array_equal(moved, (w != p).any(1)) and 20 <= moved.sum() <= 480


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: the box rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_box_rule(pkg):
    """every face, the lowest-axis tie, q_j = 0 (and -0), a point on the surface and one outside (neither moved), the centre at the
    frame's pivot, and a quarter turn that sends the local x axis to the world's y axis"""
    h = [0.3, 0.2, 0.5, 0.0]
    cases = [([0.25, 0.0, 0.0], [0.3, 0.0, 0.0]), ([-0.25, 0.05, 0.1], [-0.3, 0.05, 0.1]),
             ([0.0, 0.15, 0.0], [0.0, 0.2, 0.0]), ([0.1, -0.15, -0.2], [0.1, -0.2, -0.2]),
             ([0.0, 0.0, 0.45], [0.0, 0.0, 0.5]), ([0.1, 0.05, -0.45], [0.1, 0.05, -0.5]),
             ([0.0, 0.0, 0.0], [0.0, 0.2, 0.0]),                                       # the centre: least depth along y, d_y = 0 counts as >= 0
             ([0.0, -0.0, 0.0], [0.0, 0.2, 0.0]),
             ([0.28, 0.0, 0.0], [0.3, 0.0, 0.0]), ([0.0, 0.19, 0.0], [0.0, 0.2, 0.0])]
    for p, want in cases:
        got, moved = pkg.shape_query(BOX, h, [p])
        assert moved[0] and np.array_equal(got[0], np.array(want)), (p, got)
    for p in ([0.3, 0.1, 0.1], [-0.3, 0.0, 0.0], [0.0, 0.2, 0.4], [0.1, 0.1, -0.5], [0.4, 0.0, 0.0], [0.0, -0.7, 0.0], [0.31, 0.21, 0.51]):
        got, moved = pkg.shape_query(BOX, h, [p])
        assert not moved[0] and np.array_equal(got[0], np.array(p)), (p, got)      # on the surface or outside: untouched
    cube = [0.5, 0.5, 0.5, 0.0]
    for p, want in (([0.25, 0.25, 0.1], [0.5, 0.25, 0.1]), ([0.0, 0.25, -0.25], [0.0, 0.5, -0.25]), ([0.25, -0.25, 0.25], [0.5, -0.25, 0.25]),
                    ([-0.25, 0.1, 0.25], [-0.5, 0.1, 0.25])):
        got, moved = pkg.shape_query(BOX, cube, [p])                                 # ties go to the lowest axis
        assert moved[0] and np.array_equal(got[0], np.array(want)), (p, got)
    o = np.array([1.0, 2.0, 3.0])
    got, moved = pkg.shape_query(BOX, h, [o + [0.25, 0, 0], o + [0.0, 0.0, -0.45], [0.0, 0.0, 0.0]], _frame(np.eye(3), o))
    assert moved.tolist() == [True, True, False]
    assert np.array_equal(got, np.array([o + [0.3, 0, 0], [1.0, 2.0, 2.5], [0.0, 0.0, 0.0]]))
    f = _frame(_quarter(2, 1), o)                                                   # local x -> world y
    got, moved = pkg.shape_query(BOX, h, [o + [0.0, 0.25, 0.0], o + [0.25, 0.0, 0.0], o + [-0.15, 0.0, 0.0]], f)
    assert moved.tolist() == [True, False, True]
    want = np.array([o + [0.0, 0.3, 0.0], o + [0.25, 0.0, 0.0], o + [-0.2, 0.0, 0.0]])
    assert np.abs(got - want).max() <= 4 * EPS * 3.0 and np.array_equal(got[1], want[1])      # (two sums with o, |o_j| <= 3, round on the way there and back)
    for bad in ([0.0, 0.2, 0.5, 0], [0.3, -0.2, 0.5, 0], [0.3, 0.2, np.inf, 0], [np.nan, 0.2, 0.5, 0]):
        _expect(pkg, lambda: pkg.shape_query(BOX, bad, [[0.0, 0, 0]]), "error 1")
    _expect(pkg, lambda: pkg.shape_query(MESH, h, [[0.0, 0, 0]]), "error 1")
    _expect(pkg, lambda: pkg.shape_query(BOX, h, [[0.0, 0, 0]], _frame(2 * np.eye(3), o)), "error 1")


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: admm_hip_mesh_query_framed against a mesh created from pre-rotated vertices
# ---------------------------------------------------------------------------------------------------------------------------------
def _tetrahedron():
    """a regular tetrahedron with every face split at its centroid: 12 triangles"""
    V = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * 0.4
    F0 = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    V2, F = list(V), []
    for a, b, c in F0:
        V2.append((V[a] + V[b] + V[c]) / 3)
        k = len(V2) - 1
        F += [[a, b, k], [b, c, k], [c, a, k]]
    return orient(np.array(V2), np.array(F, dtype=np.int32))


def _octahedron():
    V = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.5
    F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    return orient(V, F)


def _small_mesh(name):
    if name == "cube":
        V, F = mesh("cube")
        return V * 0.7 - 0.35, F
    return _tetrahedron() if name == "tetrahedron" else _octahedron()


MARGIN = 1e-3      # of the mesh's extent: the nearest feature of a test point is nearer than any other triangle's closest point by at least this


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "octahedron"])
def test_mesh_query_framed_vs_prerotated_mesh(pkg, name):
    """A framed instance (translation t, then R about o) against admm_hip_mesh_query on a mesh created from the vertices
    o + R (V + t - o).  Points: over the inside of a face (barycentric weights >= 0.2 of the face's own corners, so nearer to its plane
    than to any other), 0.03 of the extent outside and inside it; a brute force over all triangles confirms that the closest point's
    triangle -- or, on a split face, its coplanar neighbours with the same closest point -- beats every other closest point by MARGIN.
    The sign agrees and the closest points agree within 32 eps (|p - o| + |q' - o| + extent + |o|): the bound of
    test_shape_query_vs_longdouble, whose stages the framed query shares, with the mesh's extent added to the scale for the closest
    point's own arithmetic and for the rounding of the pre-rotated vertices, and a factor two for those two further stages."""
    V, F = _small_mesh(name)
    assert 8 <= len(F) <= 20
    rng = np.random.default_rng(31)
    ext = (V.max(0) - V.min(0)).max()
    t = np.array([0.3, -0.2, 0.1])
    worst = 0.0
    for R, o in ((_rot([1.0, 2.0, -1.0], 0.8), np.array([0.2, 0.5, -0.3])), (_quarter(1, 1), np.array([-1.0, 0.4, 0.0])), (_rot([0.0, 1.0, 1.0], 2.5), np.array([600.0, -700.0, 400.0]))):
        f = _frame(R, o)
        A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        nrm = np.cross(B - A, C - A)
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        w = rng.dirichlet([1, 1, 1], (len(F), 6)) * 0.4 + 0.2                       # weights in [0.2, 0.6], summing to 1
        base = np.einsum("fk,fj->fkj", w[:, :, 0], A) + np.einsum("fk,fj->fkj", w[:, :, 1], B) + np.einsum("fk,fj->fkj", w[:, :, 2], C)
        side = np.where(np.arange(6) % 2 == 0, 1.0, -1.0)
        loc = (base + 0.03 * ext * side[None, :, None] * nrm[:, None, :]).reshape(-1, 3)
        # the margin, by brute force in local coordinates
        npt, nt = len(loc), len(F)
        cp = _closest_on_tris(np.repeat(loc, nt, 0), np.tile(A, (npt, 1)), np.tile(B, (npt, 1)), np.tile(C, (npt, 1))).reshape(npt, nt, 3)
        d = np.linalg.norm(cp - loc[:, None, :], axis=2)
        best = d.argmin(1)
        other = np.linalg.norm(cp - cp[np.arange(len(loc)), best][:, None, :], axis=2) > 1e-9 * ext
        assert (np.where(other, d, np.inf).min(1) - d.min(1) >= MARGIN * ext).all()
        P = _to_world(f.astype(L), (loc + t).astype(L)).astype(np.float64)
        Vw = _to_world(f.astype(L), (V + t).astype(L)).astype(np.float64)
        proj, sd = pkg.mesh_query(V, F, P, t, frame=f)
        wproj, wsd = pkg.mesh_query(Vw, F, P)
        assert np.array_equal(sd > 0, wsd > 0) and np.array_equal(sd > 0, np.tile(side < 0, len(F)))
        q2 = _to_local(f.astype(L), proj.astype(L)).astype(np.float64)
        tol = 32 * EPS * (np.linalg.norm(P - o, axis=1) + np.linalg.norm(q2 - o, axis=1) + ext + np.linalg.norm(o))
        err = np.abs(proj - wproj).max(1)
        assert (err <= tol).all(), (err / tol).max()
        assert np.abs(np.abs(sd) - 0.03 * ext).max() <= 1e-9 * max(1.0, np.linalg.norm(o))
        worst = max(worst, (err / tol).max())
        # no frame, or the identity: the bits of admm_hip_mesh_query
        a = pkg.mesh_query(V, F, P, t)
        for ff in (IDENT, _frame(np.eye(3), o)):
            b = pkg.mesh_query(V, F, P, t, frame=ff)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    print("%s: framed query vs pre-rotated mesh, worst error / bound %.3g" % (name, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 4: the refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_frame_argument_checks(pkg):
    """a host-only context: every refusal of admm_hip_set_collision_frames and of admm_hip_set_collision_shapes for a box, each naming
    its entry; a refused call leaves the previous frames in force (seen through which lists are then accepted or refused); the frames
    a new list keeps (the same length) or loses (another length)"""
    mg = pkg.meshgen
    xb, tets = mg.bar(1, 1, 1)
    x = np.concatenate([xb, np.random.default_rng(0).uniform(-1, 2, size=(40, 3))])
    s = pkg.System(device_id=-1)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    sid = s.add_body_surface(0, len(xb), mg.tet_surface(tets))
    floor, box, body = [0, -1, 0, 0], [0.3, 0.2, 0.5, 0], [0, 0, 0, sid]
    _expect(pkg, lambda: s.set_collision_shapes([FLOOR, BOX], [floor, [0.3, 0.0, 0.5, 0]]), "error 1", "shape 1", "half extent 1", "positive")
    _expect(pkg, lambda: s.set_collision_shapes([BOX, FLOOR], [[-0.3, 0.2, 0.5, 0], floor]), "error 1", "shape 0", "half extent 0")
    _expect(pkg, lambda: s.set_collision_shapes([FLOOR, FLOOR, BOX], [floor, floor, [0.3, 0.2, np.inf, 0]]), "error 1", "shape 2", "half extent 2")
    _expect(pkg, lambda: s.set_collision_shapes([BOX], [[np.nan, 0.2, 0.5, 0]]), "error 1", "shape 0")
    _expect(pkg, lambda: s.set_collision_shapes([5], [floor]), "type 5")
    s.set_collision_shapes([FLOOR, BOX, MESH], [floor, box, body])
    turn = _frame(_rot([0, 0, 1.0], 0.3), [0.1, 0.2, 0.3])
    moved_box = _frame(np.eye(3), [0.5, 0.5, 0.5])                                   # the identity rotation: a pivot alone is no frame
    _expect(pkg, lambda: s.set_collision_frames([turn, IDENT]), "error 1", "2 frames", "3 entries")
    bad = turn.copy(); bad[10] = np.inf
    _expect(pkg, lambda: s.set_collision_frames([IDENT, bad, IDENT]), "error 1", "shape 1", "component 10", "not finite")
    bad = turn.copy(); bad[4] = np.nan
    _expect(pkg, lambda: s.set_collision_frames([bad, IDENT, IDENT]), "error 1", "shape 0", "not finite")
    _expect(pkg, lambda: s.set_collision_frames([IDENT, _frame(1.001 * np.eye(3), [0, 0, 0]), IDENT]), "error 1", "shape 1", "not a rotation", "R^T R")
    shear = np.eye(3); shear[0, 1] = 1e-9
    _expect(pkg, lambda: s.set_collision_frames([_frame(shear, [0, 0, 0]), IDENT, IDENT]), "error 1", "shape 0", "not a rotation")
    _expect(pkg, lambda: s.set_collision_frames([IDENT, IDENT, _frame(np.diag([1.0, 1.0, -1.0]), [0, 0, 0])]), "error 1", "shape 2", "not a rotation", "det")
    _expect(pkg, lambda: s.set_collision_frames([turn, moved_box, turn]), "error 1", "shape 2", "body surface")
    s.set_collision_frames([IDENT, turn, moved_box])                                 # a body surface takes the identity rotation with any pivot
    # a refused call left (I, turn, I) in force: the same length keeps them, so the body surface may not move to entry 1 ...
    _expect(pkg, lambda: s.set_collision_frames([turn, turn, turn]), "shape 2", "body surface")
    _expect(pkg, lambda: s.set_collision_shapes([FLOOR, MESH, BOX], [floor, body, box]), "error 1", "shape 1", "body surface", "frame")
    s.set_collision_shapes([MESH, FLOOR, BOX], [body, floor, box])                   # ... but to entry 0, which the refused call would have turned
    s.set_collision_shapes([FLOOR, BOX, MESH], [floor, box, body])
    # another length resets them: back at three entries every order is accepted
    s.set_collision_shapes([FLOOR, BOX], [floor, box])
    s.set_collision_shapes([FLOOR, MESH, BOX], [floor, body, box])
    s.set_collision_frames([turn, IDENT, turn])
    s.set_collision_frames(None)                                                     # NULL: every entry back to the identity
    s.set_collision_shapes([MESH, FLOOR, BOX], [body, floor, box])
    # after finalize: the call's own checks again, and a kept frame that would land on the body surface
    s.set_collision_shapes([FLOOR, BOX, MESH], [floor, box, body])
    s.set_collision_frames([turn, turn, IDENT])
    s.initialize()
    _expect(pkg, lambda: s.set_collision_frames([IDENT, IDENT, turn]), "shape 2", "body surface")
    _expect(pkg, lambda: s.set_collision_frames([IDENT]), "1 frames", "3 entries")
    _expect(pkg, lambda: s.set_collision_shapes([MESH, BOX, FLOOR], [body, box, floor]), "shape 0", "body surface")
    s.set_collision_frames(None)
    s.set_collision_shapes([MESH, BOX, FLOOR], [body, box, floor])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 5: the framed kernel against the host routines, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
N_NODES = 65      # one full 64-lane block and one lane of a second
MESH_NAMES = ["tetrahedron", "cube", "octahedron"]


def _mesh_vel(V, k):
    return np.stack([0.6 * np.sin(3 * V[:, 1] + k) + 0.4 * V[:, 2], -0.5 * V[:, 0] * V[:, 2] + 0.2, 0.7 * np.cos(2 * V[:, 0]) - 0.3 * k], 1)      # not rigid


def _entry(rng, ty, k, framed):
    """one list entry among the candidates of _case: (type, params, frame, mu, motion)"""
    c = rng.uniform(-0.4, 0.4, 3)
    if ty == FLOOR:
        par = [0.0, rng.uniform(-0.6, -0.4), 0.0, 0.0]
    elif ty in (SPHERE, CYLINDER):
        par = [*c, rng.uniform(0.35, 0.55)]
    elif ty == BOX:
        par = [*rng.uniform(0.2, 0.45, 3), 0.0]
    else:
        par = [*c, float(k % 3)]
    if framed:      # the pivot near the shape, so that the turned shape stays among the candidates; a floor turned by 0.6 at most (it stays a floor)
        ang = rng.uniform(0.3, 2.8) if ty != FLOOR else rng.uniform(0.2, 0.6)
        pivot = c if ty == BOX else (c + rng.uniform(-0.15, 0.15, 3) if ty != FLOOR else rng.uniform(-0.2, 0.2, 3))
        f = _frame(_rot(rng.normal(size=3), ang) if k % 4 or ty == FLOOR else _quarter(k % 3, 1 + k % 2), pivot)
    else:
        f = _frame(np.eye(3), c if ty == BOX else np.zeros(3))
    mu = [0.3, 0.0, 0.7, np.inf, 0.15][k % 5]
    motion = np.concatenate([rng.uniform(-0.8, 0.8, 3), rng.uniform(-2.5, 2.5, 3), rng.uniform(-0.5, 0.5, 3)]) if k % 3 != 1 else np.zeros(9)
    return ty, par, f, mu, motion


def _lists():
    """the two lists of the GPU tests: five entries, one of each type, all framed; and ADMM_MAX_SHAPES = 64 entries cycling through the
    types, three of four framed"""
    rng = np.random.default_rng(41)
    short = [_entry(rng, ty, k, True) for k, ty in enumerate([FLOOR, SPHERE, CYLINDER, BOX, MESH])]
    short[4] = (MESH, [*short[4][1][:3], 1.0], *short[4][2:])                       # the cube
    rng = np.random.default_rng(42)
    full = [_entry(rng, [SPHERE, BOX, MESH, CYLINDER, FLOOR][k % 5], k, k % 4 != 3) for k in range(64)]
    return {"short": short, "full": full}


def _host_compose(pkg, entries, p, x0, friction, moving):
    """the list's entries in order on the host: shape_query or mesh_query_framed, then the friction rule on the world-space points ->
    (z, how many pushes, modes of the friction applications at pushes)"""
    meshes = [pkg.Mesh(*_small_mesh(nm)) for nm in MESH_NAMES]
    pushes, modes = 0, []
    for ty, par, f, mu, motion in entries:
        vi = None
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
        else:
            mi = int(par[3])
            proj, sd = meshes[mi].query(p, par[:3], frame=f)
            moved = sd > 0
            q = np.where(moved[:, None], proj, p)
            if moving:                                                              # the vertex velocities at the hit, in the mesh's own coordinates, turned by R
                framed = not np.array_equal(f[:9], IDENT[:9])
                loc = _to_local(f, p) if framed else p
                vi, _, _ = pkg.mesh_velocity_query(meshes[mi], None, loc, _mesh_vel(_small_mesh(MESH_NAMES[mi])[0], mi), par[:3])
                if framed:
                    vi = _rotate(f, vi)
        assert np.array_equal(moved, (q != p).any(1))
        pushes += int(moved.sum())
        if friction:
            w = _np_rigid(motion if moving else np.zeros(9), q)
            if vi is not None:
                w = w + DT * vi
            q2, mode = (pkg.friction_query_moving(p, q, x0, w, mu) if moving else pkg.friction_query(p, q, x0, mu))
            modes.append(mode[moved])
            q = q2
        p = q
    return p, pushes, (np.concatenate(modes) if modes else np.zeros(0, np.int32))


def _case():
    """test_collision_friction's candidates drawn together by 0.6 (within about 0.8 of the origin), so that every small shape holds a few"""
    dx, x0, u = _kernel_case(N_NODES, 5)
    return 0.6 * dx, 0.6 * x0, 0.6 * u


def _framed_system(pkg, entries, x0, friction, moving):
    types = [e[0] for e in entries]
    mu = [e[3] if friction else 0.0 for e in entries]
    s, b = _points_system(pkg, x0, types, [e[1] for e in entries], mu, meshes=[_small_mesh(nm) for nm in MESH_NAMES])
    s.set_collision_frames([e[2] for e in entries])
    if moving:
        s.set_collision_motion([e[4] for e in entries])
        for mi, nm in enumerate(MESH_NAMES):
            s.set_collision_mesh_velocity(mi, _mesh_vel(_small_mesh(nm)[0], mi))
    return s, b


def _framed_step(pkg, which, friction, moving):
    entries = _lists()[which]
    dx, x0, u = _case()
    s, b = _framed_system(pkg, entries, x0, friction, moving)
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    return entries, dx, x0, u, r["z"].copy(), r["u"].copy()


def test_framed_case_counts(pkg):
    """the seeds of the GPU kernel tests, checked on the host: every entry type pushes some of the 65 candidates in both lists, and with
    friction there are contacts that stick and contacts that slip"""
    dx, x0, u = _case()
    for which, entries in _lists().items():
        assert len(entries) == (64 if which == "full" else 5) and {e[0] for e in entries} == {FLOOR, SPHERE, CYLINDER, BOX, MESH}
        for ty in (FLOOR, SPHERE, CYLINDER, BOX, MESH):
            sub = [e for e in entries if e[0] == ty and not np.array_equal(e[2][:9], IDENT[:9])]
            assert sum(_host_compose(pkg, [e], dx + u, x0, False, False)[1] for e in sub) >= 3, (which, ty)
        for moving in (False, True):
            _, _, modes = _host_compose(pkg, entries, dx + u, x0, True, moving)
            assert (modes == 1).sum() >= 3 and (modes == 2).sum() >= 3, (which, moving, [int((modes == k).sum()) for k in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "friction", "moving"])
@pytest.mark.parametrize("which", ["short", "full"])
def test_kernel_equals_host_composition(pkg, which, case):
    """65 nodes, one local step of the collision batch alone: z and u bitwise equal to the host composition of admm_hip_shape_query,
    admm_hip_mesh_query_framed and the friction queries, for the five-entry list (a framed floor, sphere, cylinder, box and cube mesh)
    and the 64-entry list -- without friction, with friction, and with a rigid motion on the entries and vertex velocities on the framed
    meshes.  Fails without the feature: the frames and the box do not exist there."""
    friction, moving = case != "plain", case == "moving"
    entries, dx, x0, u, z, un = _framed_step(pkg, which, friction, moving)
    want, pushes, modes = _host_compose(pkg, entries, dx + u, x0, friction, moving)
    print("%s list, %s: %d pushes, none / stick / slip %s" % (which, case, pushes, [int((modes == k).sum()) for k in range(3)]))
    assert pushes >= 20
    assert np.array_equal(z, want), (np.abs(z - want).max(), np.count_nonzero((z != want).any(1)))
    assert np.array_equal(un, u + (dx - want))
    if moving:                                                                      # and the motion matters
        still, _, _ = _host_compose(pkg, entries, dx + u, x0, True, False)
        assert np.abs(still - want).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 6: identity frames are the existing path
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_identity_frames_are_the_existing_path(pkg):
    """frames set to the identity on every entry (with pivots, before and after initialize, and a turn set and taken back): z and u of
    the four-shape kernel scene, and x, v, u, z of the tet bar over three frames, bitwise those of a context that never made the call;
    admm_hip_debug_graph_state is the same"""
    from test_moving_friction import _rigid_system
    dx, x0, u = _kernel_case(200, 3)
    outs = []
    for variant in range(3):
        s, b = _rigid_system(pkg, x0)
        if variant == 1:
            s.set_collision_frames([_frame(np.eye(3), [k, -k, 0.5]) for k in range(4)])
        if variant == 2:
            s.set_collision_frames([_frame(_rot([1, 1, 0], 0.4), [0, 0, 0])] * 4)
            s.write_local(b, u=u); s.local_step_dx(b, dx)
            s.set_collision_frames(None)
        s.write_local(b, u=u)
        s.local_step_dx(b, dx)
        r = s.read_local(b)
        outs.append((r["z"].copy(), r["u"].copy()))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
    a = _bar(pkg); a.initialize()
    fa = _bar_frames(a, 3)
    b = _bar(pkg); b.set_collision_frames([IDENT, _frame(np.eye(3), [0.2, 0.1, 0.0])]); b.initialize()
    b.set_collision_frames([IDENT, IDENT])
    fb = _bar_frames(b, 3)
    assert _same(fa, fb)
    assert a.graph_state() == b.graph_state(), (a.graph_state(), b.graph_state())


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 8 (and the scene of 7): a block on a ramp
# ---------------------------------------------------------------------------------------------------------------------------------
THETA = np.deg2rad(20.0)
BLOCK = (2, 1, 2)      # 4 cells, 24 tets or fewer


def _block_system(pkg, x, gravity, frame, mu, springs=False):
    mg = pkg.meshgen
    xr, tets = mg.bar(*BLOCK)
    m = mg.lumped_tet_mass(xr, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    if springs:                                                                     # a second batch: the fused whole-scene launch then runs, beside the collision batch's own
        s.add_forces(KIND["SPRING"], np.array([[0, len(x) - 1], [1, len(x) - 2]], dtype=np.int32), [50.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity(gravity)
    s.set_collision_shapes([FLOOR], [[0, 0, 0, 0]])
    if frame is not None:
        s.set_collision_frames([frame])
    s.set_collision_friction([mu])
    s.initialize()
    s.mass = m
    return s


def _block_frames(s, frames=10, iters=20):
    out = []
    for _ in range(frames):
        s.step(iters)
        out.append(s.m_x.reshape(-1, 3).copy())
    return np.array(out)


def _ramp_runs(pkg, mu):
    """-> (the block on the framed floor, the block on the level floor under turned gravity turned back, that run's sensitivity)"""
    X, _ = pkg.meshgen.bar(*BLOCK)
    R = _rot([0, 0, 1.0], THETA)
    g = np.array([0.0, -G, 0.0])
    framed = _block_frames(_block_system(pkg, X @ R.T, g, _frame(R, [0, 0, 0]), mu))
    flat = _block_frames(_block_system(pkg, X, R.T @ g, None, mu))
    pert = _block_frames(_block_system(pkg, (X @ R.T) @ R, R.T @ g, None, mu))    # there and back: a rounding-level perturbation of X
    return framed, flat @ R.T, np.abs(pert - flat).max()


def _along(xs, m):
    """the centre of mass's travel along the slope from the first frame to the last"""
    t = _rot([0, 0, 1.0], THETA) @ np.array([1.0, 0, 0])
    com = (m[:, None] * (xs[-1] - xs[0])).sum(0) / m.sum()
    return abs(float(com @ t))


@pytest.mark.gpu
def test_ramp_against_rotated_gravity(pkg):
    """A 2 x 1 x 2-cell block of LinearTetStrain tets on the floor y = 0 turned by 20 degrees about z, gravity -y, 10 frames of 20
    iterations, against the same block on the unframed floor under gravity turned by -20 degrees, that result turned back.  The allowed
    difference is ten times the unframed run's own sensitivity: the same level scene started from positions turned by R and back.
    Measured on the MI355X (max over the ten frames and all coordinates):
        mu = 0          sensitivity 3.664e-15, framed against turned gravity 7.262e-15
        mu = 2 tan 20   sensitivity 1.804e-16, framed against turned gravity 2.914e-16
    and the travel along the slope 0.07379 (mu = 0), 2.530e-04 (mu = 2 tan 20), 0.03695 (mu = tan 20 / 2).
    With mu = 2 tan(theta) the centre of mass moves along the slope by less than a tenth of what it moves without friction (stick is no
    tangential motion at all; the margin covers the unconverged iterations), with mu = tan(theta) / 2 by more than a tenth."""
    m = None
    travel = {}
    for mu in (0.0, 2 * np.tan(THETA)):
        framed, flat_back, sens = _ramp_runs(pkg, mu)
        diff = np.abs(framed - flat_back).max()
        print("ramp, mu = %.4f: sensitivity of the unframed run %.3e, framed against turned gravity %.3e" % (mu, sens, diff))
        assert sens > 0 and diff <= 10 * sens, (mu, diff, sens)
        if m is None:
            X, tets = pkg.meshgen.bar(*BLOCK)
            m = pkg.meshgen.lumped_tet_mass(X, tets, 1000.0)
        X0 = X @ _rot([0, 0, 1.0], THETA).T
        travel[mu] = _along(np.concatenate([X0[None], framed]), m)
    R = _rot([0, 0, 1.0], THETA)
    half = _block_frames(_block_system(pkg, X @ R.T, np.array([0.0, -G, 0.0]), _frame(R, [0, 0, 0]), 0.5 * np.tan(THETA)))
    travel["half"] = _along(np.concatenate([(X @ R.T)[None], half]), m)
    print("ramp: travel along the slope, mu = 0: %.5f, 2 tan: %.3e, tan / 2: %.5f" % (travel[0.0], travel[2 * np.tan(THETA)], travel["half"]))
    assert travel[0.0] > 0.03
    assert travel[2 * np.tan(THETA)] < 0.1 * travel[0.0]
    assert travel["half"] > 0.1 * travel[0.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 7: the per-batch launch path, in a child process
# ---------------------------------------------------------------------------------------------------------------------------------
def _launch_path_results(pkg):
    """what the parent and the child both compute: the scenes of test 5 (the moving case, both lists), and three frames of the ramp
    block with a spring batch beside its tets, so that a default context runs the fused whole-scene launch"""
    out = {}
    for which in ("short", "full"):
        _, _, _, _, z, un = _framed_step(pkg, which, True, True)
        out["z_" + which], out["u_" + which] = z, un
    X, _ = pkg.meshgen.bar(*BLOCK)
    R = _rot([0, 0, 1.0], THETA)
    s = _block_system(pkg, X @ R.T, np.array([0.0, -G, 0.0]), _frame(R, [0, 0, 0]), 0.2, springs=True)
    out["ramp"] = _block_frames(s, 3)
    return out


def _child_main(path):
    from __graft_entry__ import load_package
    np.savez(path, **_launch_path_results(load_package()))


@pytest.mark.gpu
def test_per_batch_path_gives_the_same_bits(pkg, tmp_path):
    """ADMM_HIP_LOCAL_MULTI=0 in a fresh child process: the scenes of test_kernel_equals_host_composition and three frames of the ramp
    block (tets, springs and the framed floor: by default the fused launch plus the collision batch's own) give the parent's bits"""
    want = _launch_path_results(pkg)
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, ADMM_HIP_LOCAL_MULTI="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_collision_frames as t; t._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.load(path)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    assert np.abs(want["ramp"][-1] - want["ramp"][0]).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 9: the class API
# ---------------------------------------------------------------------------------------------------------------------------------
CPP_BOX = dict(c=[0.3, -0.25, 0.05], h=[0.3, 0.1, 0.3], R=_rot([0.2, 0.1, 1.0], 0.3))
CPP_CYL = dict(c=[-0.05, -0.3, 0.0], r=0.2, R=_rot([1.0, 0.0, 0.0], 1.2), o=[0.0, -0.3, 0.0])


def test_cpp_frames_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_frames", pkg))


@pytest.mark.gpu
def test_class_api_box_and_oriented_cylinder(pkg, tmp_path):
    """a CollisionBox turned about its centre and a CollisionCylinder with an orientation in one CollisionForce, through admm::System:
    the block's frames bitwise equal to the same scene set up through the C ABI; it lands on the box"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_frames", pkg)
    mg = pkg.meshgen
    x, tets = mg.bar(*BLOCK)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(tets)], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f); tets.astype(np.int32).tofile(f)
        np.concatenate([CPP_BOX["c"], CPP_BOX["h"], CPP_BOX["R"].ravel(), CPP_CYL["c"], [CPP_CYL["r"]], CPP_CYL["R"].ravel(), CPP_CYL["o"], [0.4]]).tofile(f)
    frames = 12
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [32.0])
    s.add_gravity([0.0, -G, 0.0])
    s.set_collision_shapes([BOX, CYLINDER], [[*CPP_BOX["h"], 0.0], [CPP_CYL["c"][0], CPP_CYL["c"][1], 0.0, CPP_CYL["r"]]])
    s.set_collision_frames([_frame(CPP_BOX["R"], CPP_BOX["c"]), _frame(CPP_CYL["R"], CPP_CYL["o"])])
    s.set_collision_friction([0.4, 0.0])
    s.initialize()
    want = _block_frames(s, frames).reshape(frames, -1)
    r = subprocess.run([exe, inp, out, str(frames), "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(out).reshape(frames, -1)
    assert np.array_equal(got, want), np.abs(got - want).max()
    free = x.ravel() + np.concatenate([[0.0, -0.5 * G * (frames * DT) * ((frames + 1) * DT), 0.0]] * len(x))
    assert np.abs(want[-1] - free).max() > 1e-2                                     # the fall was stopped
