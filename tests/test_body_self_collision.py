"""Self-collision of a closed body surface (extension, no reference counterpart): the surface nodes of a tet body meet their own skin
outside what is near them in the rest shape (admm_hip_set_body_self_collision, project_collision_bodyself_kernel; csrc/mesh_query.hpp:
rest_near, closest_within_rest_excluding, body_self_project).

CPU: the host rule against an np.longdouble brute force and a float64 restatement; the reductions; the refusals.  GPU: the kernel bit
for bit against the host composition; off changes nothing; a slotted bar closing on itself; launch modes, two shards, the class API.

The surfaces are meshgen.slotted_bar(nx, ny, nz, 2, h = 0.1) with the lengths r = 0.2 h, R = 0.5 h, rho = 0.9 h: two arms one cell apart
joined by a spine.  (3, 3, 8, 2) has 144 nodes, 140 on the surface and 4 inside (three 64-lane blocks, the last one partial)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from checkers import KIND
from test_collision_friction import DT, W
from test_collision_frames import IDENT, _frame, _rot
from test_collision_mesh import FLOOR, MESH, _closest_on_tris
from test_collision_shell import _cube, _extent, _grid, _same_frames
from test_moving_friction import _np_rigid

L = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADMM_ERR_ARG, ADMM_ERR_STATE = 1, 3

H = 0.1
SLOT = 2
R_GAP, REACH, RHO = 0.2 * H, 0.5 * H, 0.9 * H
LENGTHS = (R_GAP, REACH, RHO)


def _surface(pkg, dims):
    """-> dict: x [n][3] and tets of slotted_bar(*dims, SLOT, H); F the surface in node ids; sv the surface nodes ascending (vertex k is
    node sv[k], the numbering admm_hip_add_body_surface fixes); vid [n] the vertex id of every node (-1: interior); V = x[sv] the rest
    vertices, Fl the surface in vertex ids"""
    mg = pkg.meshgen
    x, tets = mg.slotted_bar(*dims, SLOT, H)
    F = mg.tet_surface(tets, x)
    sv = np.unique(F)
    vid = np.full(len(x), -1, np.int32); vid[sv] = np.arange(len(sv), dtype=np.int32)
    return dict(x=x, tets=tets, F=F, sv=sv, vid=vid, V=np.ascontiguousarray(x[sv]), Fl=np.ascontiguousarray(vid[F], dtype=np.int32))


def _upper(P):
    """the upper arm: beyond the spine, above the slot's middle"""
    return (P[:, 1] > 1.5 * H) & (P[:, 2] > SLOT * H + 1e-9)


def _closed(V):
    """the rest vertices with the upper arm shifted down by h, onto the lower arm"""
    cur = V.copy()
    cur[_upper(V), 1] -= H
    return cur


def _lowest_first(F):
    k = F.argmin(1)
    return np.stack([F[np.arange(len(F)), (k + j) % 3] for j in range(3)], 1)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def _pseudo_normals(V, F):
    """np.longdouble: unit face normals [nt][3], the unit edge normals by sorted vertex pair, the unit angle-weighted vertex normals"""
    Vl = V.astype(L)
    A, B, C = Vl[F[:, 0]], Vl[F[:, 1]], Vl[F[:, 2]]
    fn = _unit(np.cross(B - A, C - A))
    en, vn = {}, np.zeros((len(V), 3), L)
    for t in range(len(F)):
        for k in range(3):
            a, b, c = F[t, k], F[t, (k + 1) % 3], F[t, (k + 2) % 3]
            key = (min(a, b), max(a, b))
            en[key] = en.get(key, 0) + fn[t]
            e1, e2 = _unit(Vl[b] - Vl[a]), _unit(Vl[c] - Vl[a])
            vn[a] += np.arccos(np.clip((e1 * e2).sum(), -1, 1)) * fn[t]
    return fn, {k: _unit(v) for k, v in en.items()}, _unit(vn)


def _brute_self(cur, X, F, P, vid, rho, ext):
    """np.longdouble, exhaustive: for every point (vertex vid[i], vid >= 0) the winner among the triangles whose rest distance to
    X[vid[i]] is >= rho -> dict(c, d, tri, co, spread, g, rest_gap): closest point, distance, triangle, the co-winners, g against
    the angle-weighted pseudo-normal of the closest point's feature (recomputed from cur), the smallest |rest distance - rho|"""
    npt, nt = len(P), len(F)
    Pl, Cl, Xl = P.astype(L), cur.astype(L), X.astype(L)

    def all_d2(Q, Vv):
        A, B, C = Vv[F[:, 0]], Vv[F[:, 1]], Vv[F[:, 2]]
        cp = _closest_on_tris(np.repeat(Q, nt, 0), np.tile(A, (len(Q), 1)), np.tile(B, (len(Q), 1)), np.tile(C, (len(Q), 1))).reshape(len(Q), nt, 3)
        return cp, ((cp - Q[:, None, :]) ** 2).sum(2)
    _, rest_d2 = all_d2(Xl[vid], Xl)
    rest_d = np.sqrt(rest_d2)
    cp, d2 = all_d2(Pl, Cl)
    d2 = np.where(rest_d < L(rho), L(np.inf), d2)
    tri = d2.argmin(1)
    ar = np.arange(npt)
    best = d2[ar, tri]
    c = cp[ar, tri]
    fn, en, vn = _pseudo_normals(cur, F)
    tol = L(1e-12) * L(ext)
    g = np.zeros(npt, L)
    for i in range(npt):
        T = F[tri[i]]
        on = [np.sqrt(((c[i] - Cl[T[k]]) ** 2).sum()) < tol for k in range(3)]
        n = None
        if any(on):
            n = vn[T[on.index(True)]]
        else:
            for k in range(3):
                a, b = Cl[T[k]], Cl[T[(k + 1) % 3]]
                u = b - a
                s = ((c[i] - a) * u).sum() / (u * u).sum()
                if np.sqrt(((c[i] - (a + s * u)) ** 2).sum()) < tol:
                    n = en[(min(T[k], T[(k + 1) % 3]), max(T[k], T[(k + 1) % 3]))]
                    break
        if n is None:
            n = fn[tri[i]]
        g[i] = ((Pl[i] - c[i]) * n).sum()
    # triangles within the margin of the best: on a shared edge or vertex they are neighbours with one closest point, any of which is a
    # right winner (their float64 distances differ by roundings); with different closest points the winner is undecided
    co = np.sqrt(d2) <= np.sqrt(best)[:, None] + L(1e-9) * L(ext)
    spread = np.where(co, np.sqrt(((cp - c[:, None, :]) ** 2).sum(2)), 0).max(1).astype(np.float64)
    return dict(c=c, d=np.sqrt(best), tri=tri, co=co, spread=spread, g=g, rest_gap=np.abs(rest_d - L(rho)).min(1).astype(np.float64))


def _host_case(pkg, dims, seed):
    """the surface closed onto itself, its own vertices displaced by seeded uniform noise of amplitude 0.3 h, each with its id"""
    S = _surface(pkg, dims)
    cur = _closed(S["V"])
    m = pkg.Mesh(S["V"], S["Fl"])
    m.set_vertices(cur)
    P = np.ascontiguousarray(cur + np.random.default_rng(seed).uniform(-0.3 * H, 0.3 * H, cur.shape))
    return S, cur, m, P, np.arange(len(cur), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: the host rule against a brute force, and the stated order restated in float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,seed", [((2, 3, 6), 1), ((3, 3, 8), 1), ((3, 3, 8), 2)])
def test_host_rule_vs_longdouble(pkg, dims, seed):
    """Mesh.query_self against the np.longdouble brute force that leaves out by rest distance, searches the rest exhaustively and takes
    angle-weighted pseudo-normals recomputed from the current vertices.  Hit or none, collides or not, crossed or not and the winner
    are exact outside margins of 1e-9 extent on |d - r|, |d - R|, |rest d - rho|, |g| and the two best distances (two triangles within
    the margin of each other count as undecided when their closest points differ; neighbours that share the closest point, an edge or
    a vertex, are co-winners: the library's must be one of them); the share left out,
    computed from the reference alone, is at most 1 % (measured: 0 on every case); proj within 1e-12 (extent + |q|)(1 + r / d).
    Measured on (3, 3, 8), seeds 1 / 2: 23 / 21 pushed on the outside, 14 / 17 crossed, 11 / 12 hits left alone, 92 / 90 without a
    hit; worst error / bound of proj 8.1e-5 / 4.4e-5 (sdist 2.0e-5 / 1.2e-5)."""
    r, R, rho = LENGTHS
    S, cur, m, P, vid = _host_case(pkg, dims, seed)
    ext = _extent(cur)
    proj, sd, tri, cr = m.query_self(P, vid, S["V"], r, R, rho)
    ref = _brute_self(cur, S["V"], S["Fl"], P, vid, rho, ext)
    d, g = ref["d"].astype(np.float64), ref["g"].astype(np.float64)
    mar = 1e-9 * ext
    hit_ref = d < R
    sure = (np.abs(d - r) > mar) & (np.abs(d - R) > mar) & (ref["rest_gap"] > mar) & (~hit_ref | (np.abs(g) > mar)) & (~hit_ref | (ref["spread"] <= mar))
    left_out = 1.0 - sure.mean()
    crossed_ref = hit_ref & (g < 0)
    pushed_ref = hit_ref & (g >= 0) & (d < r)
    alone_ref = hit_ref & (g >= 0) & (d >= r)
    print("%s seed %d: %d vertices: %d pushed on the outside, %d crossed, %d hits left alone, %d without a hit; share left out by the margins %.4f" %
          (dims, seed, len(P), pushed_ref.sum(), crossed_ref.sum(), alone_ref.sum(), (~hit_ref).sum(), left_out))
    assert left_out <= 0.01, left_out
    if dims == (3, 3, 8):
        assert min(pushed_ref.sum(), crossed_ref.sum(), alone_ref.sum(), (~hit_ref).sum()) >= 10
    k = sure
    moved = (proj != P).any(1)
    assert np.array_equal((tri >= 0)[k], hit_ref[k]) and np.array_equal(np.isfinite(sd), tri >= 0)
    assert np.array_equal(cr.astype(bool)[k], crossed_ref[k])
    assert np.array_equal(moved[k], (pushed_ref | crossed_ref)[k])
    kh = np.flatnonzero(k & hit_ref)
    assert ref["co"][kh, tri[kh]].all()                                                 # the winner, or a neighbour that shares its closest point
    assert np.array_equal(proj[~moved], P[~moved]) and not (cr.astype(bool) & ~moved).any()
    kk = k & moved
    sign = np.where(crossed_ref, L(-1), L(1))[:, None]
    want = ref["c"] + sign * (L(r) / ref["d"])[:, None] * (P.astype(L) - ref["c"])
    first = 1e-12 * (ext + np.linalg.norm(P, axis=1))
    e_p = np.linalg.norm((proj.astype(L) - want).astype(np.float64), axis=1)[kk] / (first[kk] * (1 + r / d[kk]))
    e_sd = np.abs(sd[k & hit_ref] - np.where(crossed_ref, r + d, r - d)[k & hit_ref]) / first[k & hit_ref]
    print("%s seed %d: worst error / bound: proj %.3g, sdist %.3g" % (dims, seed, e_p.max(), e_sd.max()))
    assert e_p.max() <= 1.0 and e_sd.max() <= 1.0, (e_p.max(), e_sd.max())


def _restate_self(pkg, m, cur, X, Fl, P, vid, r, R, rho):
    """mesh_query.hpp's rule in plain float64 numpy.  The per-triangle closest points, distances and regions -- of P against the current
    triangles and of X[vid] against the rest triangles -- come from the library's closest_on_tri on one-triangle meshes (corners in the
    canonical order: lowest vertex id first); the stored pseudo-normals from Mesh.feature_normal.  Restated here: the rest test, the
    winner as the minimum of (d2, index) below R * R, the box test, g, the decision, the push and the mirror."""
    Fc = _lowest_first(Fl)
    nt, npt = len(Fc), len(P)
    one = np.array([[0, 1, 2]], np.int32)
    d2 = np.empty((npt, nt)); c = np.empty((npt, nt, 3)); reg = np.empty((npt, nt), np.int32); near = np.zeros((npt, nt), bool)
    own = vid >= 0
    for t in range(nt):
        h = pkg.Mesh(cur[Fc[t]], one, 1.0).closest(P)
        d2[:, t], c[:, t], reg[:, t] = h["d2"], h["c"], h["reg"]
        near[own, t] = pkg.Mesh(X[Fc[t]], one, 1.0).closest(X[vid[own]])["d2"] < rho * rho
    _, orig = m.boundary_table()
    slot_of = np.empty(nt, np.int32); slot_of[orig] = np.arange(nt, dtype=np.int32)
    inf = m.info()
    proj, sd, tri, cr = P.copy(), np.full(npt, -np.inf), np.full(npt, -1, np.int32), np.zeros(npt, np.int32)
    for i in np.flatnonzero(own):
        q = P[i]
        if not ((inf["lo"] - R < q) & (q < inf["hi"] + R)).all():
            continue
        ok = ~near[i] & (d2[i] < R * R)
        if not ok.any():
            continue
        t = int(np.flatnonzero(ok)[np.argmin(d2[i][ok])])                               # (argmin: the first, so the lowest index, among equals)
        cc, dd2 = c[i, t], d2[i, t]
        sl = slot_of[t:t + 1]
        n = m.feature_normal(sl, reg[i, t:t + 1])[0]
        g = (q[0] - cc[0]) * n[0] + (q[1] - cc[1]) * n[1] + (q[2] - cc[2]) * n[2]
        d = np.sqrt(dd2)
        tri[i] = t
        e = q - cc
        if not g < 0.0 or not dd2 > 0.0:
            sd[i] = r - d
            if not dd2 < r * r:
                continue
            proj[i] = cc + (r / d) * e if d > 0 else cc + r * m.feature_normal(sl, [0])[0]
        else:
            sd[i] = r + d; cr[i] = 1
            proj[i] = cc - (r / d) * e
    return proj, sd, tri, cr


@pytest.mark.parametrize("dims,seed", [((2, 3, 6), 1), ((3, 3, 8), 2)])
def test_float64_restatement_is_bitwise(pkg, dims, seed):
    r, R, rho = LENGTHS
    S, cur, m, P, vid = _host_case(pkg, dims, seed)
    got = m.query_self(P, vid, S["V"], r, R, rho)
    want = _restate_self(pkg, m, cur, S["V"], S["Fl"], P, vid, r, R, rho)
    assert got[3].sum() >= 5 and ((got[0] != P).any(1) & (got[3] == 0)).sum() >= 5
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: reductions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_reductions(pkg):
    r, R, rho = LENGTHS
    S, cur, m, P, vid = _host_case(pkg, (3, 3, 8), 1)
    # vertex_id = -1: every point is left alone
    proj, sd, tri, cr = m.query_self(P, -1, S["V"], r, R, rho)
    assert np.array_equal(proj, P) and (tri == -1).all() and not cr.any() and np.isinf(sd).all()
    # rho so small that only the 1-ring is rest-near (its rest distance is 0), r = R: a point on the outside gets the bits of
    # closest_within_excluding + shell_push, evaluated by an open mesh of the same triangles with half thickness r
    rr = 0.35 * H
    tiny = rr                                                                           # rho >= R is required; every rest distance beyond the 1-ring is >= h / sqrt(2) > tiny
    shell = pkg.Mesh(S["V"], S["Fl"], rr); shell.set_vertices(cur)
    proj, sd, tri, cr = m.query_self(P, vid, S["V"], rr, rr, tiny)
    ps, sds, tris = shell.query_excluding(P, vid)
    out = cr == 0
    assert out.sum() >= 100 and ((proj != P).any(1) & out).sum() >= 20
    assert np.array_equal(proj[out], ps[out]) and np.array_equal(tri[out], tris[out]) and np.array_equal(sd[out], sds[out])
    hit = tri >= 0
    assert not (S["Fl"][tri[hit]] == vid[hit, None]).any()
    # in the rest pose no own vertex moves
    for dims in ((2, 3, 6), (3, 3, 8), (2, 3, 8)):
        T = _surface(pkg, dims)
        proj, sd, tri, cr = pkg.Mesh(T["V"], T["Fl"]).query_self(T["V"], np.arange(len(T["V"])), T["V"], r, R, rho)
        assert np.array_equal(proj, T["V"]) and not cr.any()


def test_slotted_bar(pkg):
    mg = pkg.meshgen
    for dims, nn, inner in (((2, 3, 6, 2), 84, 2), ((3, 3, 8, 2), 144, 4)):
        x, tets = mg.slotted_bar(*dims, H)
        xb, tb = mg.bar(*dims[:3], H)
        assert np.array_equal(x, xb) and len(x) == nn and len(tets) == len(tb) - 6 * dims[0] * (dims[2] - dims[3])
        rows = {tuple(t) for t in tb}
        assert all(tuple(t) in rows for t in tets)
        F = mg.tet_surface(tets, x)
        assert len(x) - len(np.unique(F)) == inner
        pkg.Mesh(x, F)                                                                   # closed, edge-manifold, outward (validated at creation)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(pkg, rc, words, fn, *args):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*args)
    msg = str(e.value)
    assert ("error %d" % rc) in msg or ("code %d" % rc) in msg or (" %d:" % rc) in msg or (" %d " % rc) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _host_body(pkg, x=None, self_collision=None, sheet_self=False, second=False):
    """a host-only context: a cloth grid (nodes first), the slotted bar (2, 3, 6), an obstacle cube"""
    mg = pkg.meshgen
    S = _surface(pkg, (2, 3, 6))
    Vg, Fg = _grid()
    Vg = Vg + [0.0, -1.0, 0.0]
    xb = S["x"] if x is None else x
    X = np.concatenate([Vg, xb])
    s = pkg.System(device_id=-1)
    s.set_timestep(DT)
    s.add_nodes(X.ravel(), np.ones(X.size))
    s.add_forces(KIND["TRI_STRAIN"], Fg, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["TET_LINEAR"], S["tets"] + len(Vg), [2e4])
    s.add_forces(KIND["COLLISION"], np.arange(len(X), dtype=np.int32), [W])
    s.sheet = s.add_sheet_surface(0, len(Vg), Fg, 0.05, self_collision=sheet_self)
    s.body = s.add_body_surface(len(Vg), len(xb), S["F"] + len(Vg), self_collision=self_collision)
    Vc, Fc = _cube()
    s.cube = s.add_collision_mesh(Vc + [3.0, 0, 0], Fc)
    ids = [s.sheet, s.body, s.cube]
    if second:
        s.body2 = s.add_body_surface(len(Vg), len(xb), S["F"] + len(Vg), self_collision=self_collision)
        ids.append(s.body2)
    s.set_collision_shapes([MESH] * len(ids), [[0, 0, 0, i] for i in ids])
    return s


def test_body_self_collision_refusals(pkg):
    r, R, rho = LENGTHS
    s = _host_body(pkg)
    assert s.collision_form() == 4
    _refused(pkg, ADMM_ERR_ARG, ["collision mesh %d" % s.cube, "obstacle mesh"], s.set_body_self_collision, s.cube, r, R, rho)
    _refused(pkg, ADMM_ERR_ARG, ["collision mesh %d" % s.sheet, "sheet surface"], s.set_body_self_collision, s.sheet, r, R, rho)
    _refused(pkg, ADMM_ERR_ARG, ["not a registered mesh"], s.set_body_self_collision, 9, r, R, rho)
    for bad in ((np.nan, R, rho), (r, np.inf, rho), (r, R, np.nan)):
        _refused(pkg, ADMM_ERR_ARG, ["body surface %d" % s.body, "not finite"], s.set_body_self_collision, s.body, *bad)
    _refused(pkg, ADMM_ERR_ARG, ["body surface %d" % s.body, "reach 0.01", "below the half gap 0.02"], s.set_body_self_collision, s.body, r, 0.5 * r, rho)
    _refused(pkg, ADMM_ERR_ARG, ["body surface %d" % s.body, "rest radius 0.04", "below the reach 0.05"], s.set_body_self_collision, s.body, r, R, 0.8 * R)
    _refused(pkg, ADMM_ERR_ARG, ["body surface %d" % s.body, "negative"], s.set_body_self_collision, s.body, -r, R, rho)
    assert s.collision_form() == 4                                                      # a refused call sets nothing
    s.set_body_self_collision(s.body, r, R, rho)
    assert s.collision_form() == 7
    s.set_body_self_collision(s.body, 0.0, 0.0, 0.0)                                    # r = 0: off
    assert s.collision_form() == 4
    s.set_body_self_collision(s.body, r, R, rho)
    s.initialize()
    assert s.collision_form() == 7
    _refused(pkg, ADMM_ERR_STATE, ["before finalize"], s.set_body_self_collision, s.body, r, R, rho)
    # finalize: a body that the rule would move where it stands.  Where it was registered nothing within the reach is left in (rho >= R),
    # so this is a body that was registered open and is closed onto itself when finalize sees it: the arms' faces 0.1 h apart
    S = _surface(pkg, (2, 3, 6))
    s = _host_body(pkg, self_collision=LENGTHS)
    xc = S["x"].copy(); xc[_upper(xc), 1] -= 0.9 * H
    allx = s.m_x.reshape(-1, 3).copy(); allx[-len(xc):] = xc
    s.m_x = allx.ravel()
    _refused(pkg, ADMM_ERR_ARG, ["body surface %d" % s.body, "vertex ", "(node ", "triangle ", "distance 0.01", "rest radius 0.09", "half gap 0.02", "reach 0.05"], s.initialize)
    allx[-len(xc):] = S["x"]; s.m_x = allx.ravel()                                       # back where it was registered: accepted
    s.initialize()
    # two self-colliding surfaces over one node range: body + body, and (ranges equal) never sheet + body, which have different ranges
    s = _host_body(pkg, self_collision=LENGTHS, second=True)
    _refused(pkg, ADMM_ERR_ARG, ["surfaces %d and %d" % (s.body, s.body2), "share the node range", "one such surface"], s.initialize)
    s = _host_body(pkg, self_collision=LENGTHS, sheet_self=True)                        # a self-colliding sheet beside a self-colliding body: other nodes
    s.initialize()
    assert s.collision_form() == 7
    # the context-free query
    T = _surface(pkg, (2, 3, 6))
    m = pkg.Mesh(T["V"], T["Fl"])
    P = T["V"][:3].copy()
    m.query_self(P, [len(T["V"]) - 1, -1, 0], T["V"], r, R, rho)
    for bad in (len(T["V"]), -2):
        with pytest.raises(pkg.AdmmHipError):
            m.query_self(P, [0, bad, -1], T["V"], r, R, rho)
        with pytest.raises(pkg.AdmmHipError):
            m.velocity_query_self(P, [0, bad, -1], T["V"], R, rho, np.zeros_like(T["V"]))
    for bad in ((0.0, R, rho), (r, 0.5 * r, rho), (r, R, 0.5 * R), (np.nan, R, rho)):
        with pytest.raises(pkg.AdmmHipError):
            m.query_self(P, 0, T["V"], *bad)
    with pytest.raises(pkg.AdmmHipError):
        pkg.Mesh(T["V"], T["Fl"], 0.01).query_self(P, 0, T["V"], r, R, rho)              # an open mesh


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 4: the kernel against the host composition
# ---------------------------------------------------------------------------------------------------------------------------------
N_FREE = 17
CUBE_T = np.array([0.15, 0.05, 0.5])
CUBE_S = 0.12
SHELL_T = np.array([0.15, 0.26, 0.4])        # 0.06 above the closed upper arm's top face: within the reach, beyond the half thickness
R_SHELL, REACH_SHELL = 0.02, 0.1


def _kernel_scene(pkg):
    """-> (S, x0 [161][3], xc, disp): the 144 nodes of (3, 3, 8) and 17 free particles around the arms; xc: the same with the upper
    arm shifted down by h (the surface the kernel meets); disp: seeded noise of amplitude 0.3 h on the body, small on the particles"""
    S = _surface(pkg, (3, 3, 8))
    rng = np.random.default_rng(171)
    free = np.stack([rng.uniform(-0.05, 0.35, N_FREE), rng.uniform(-0.05, 0.5, N_FREE), rng.uniform(-0.05, 0.85, N_FREE)], 1)
    x0 = np.concatenate([S["x"], free])
    xc = x0.copy()
    xc[:len(S["x"])][_upper(S["x"]), 1] -= H
    disp = np.concatenate([rng.uniform(-0.3 * H, 0.3 * H, S["x"].shape), 0.02 * rng.normal(size=free.shape)])
    return S, x0, xc, disp


def _kernel_lists(framed, shell=False):
    """entries (type, params, frame, mu): [floor, the body itself (mesh 0), a closed cube (mesh 1)] and 64 entries cycling through
    them with the floor's height and the cube's place varied; framed: the floors tilted, the cubes turned; shell: a fourth entry, an
    open grid with side memory (mesh 2)"""
    rng = np.random.default_rng(172)
    fl = _frame(_rot([1.0, 0.0, 0.3], 0.05), [0.0, 0.02, 0.4]) if framed else IDENT.copy()
    fc = _frame(_rot([0.2, 1.0, -0.4], 0.8), CUBE_T + [0.02, 0.0, -0.03]) if framed else IDENT.copy()
    short = [(FLOOR, [0.0, 0.03, 0.0, 0.0], fl, 0.3), (MESH, [0.0, 0.0, 0.0, 0.0], IDENT.copy(), 0.0), (MESH, [*CUBE_T, 1.0], fc, 0.7)]
    if shell:
        return short + [(MESH, [*SHELL_T, 2.0], IDENT.copy(), 0.0)]
    full = []
    for k in range(64):
        ty, par, f, mu = short[k % 3]
        par, f = list(par), f.copy()
        d = rng.uniform(-0.1, 0.1, 3)
        if k >= 3 and k % 3 == 0:
            par[1] += 0.05 * d[1]
        if k >= 3 and k % 3 == 2:
            par[:3] = np.asarray(par[:3]) + d * [1, 0.3, 3]
            f[9:] += d * [1, 0.3, 3]
        full.append((ty, par, f, [0.3, 0.0, 0.7, np.inf, 0.15][k % 5] if k % 3 != 1 else 0.0))
    return {"short": short, "full": full}


def _kernel_compose(pkg, entries, S, body, cube, p, x0, friction, mu_s, vel, shell=None, sides=None):
    """the list on the host in its order: shape_query; for the body's entry Mesh.query_self for its own nodes (interior ones with id
    -1) and Mesh.query, the closed-mesh rule, for the free particles; Mesh.query for the cube; Mesh.query_sided for the memory shell.
    With friction the moving rule after every entry that moved a point, the body's with its own coefficient and its nodes' frame-start
    v interpolated at the winning triangle -> (z, crossed [nb], pushed [nb] by the body's entries)"""
    nb = len(S["x"])
    crossed, pushed = np.zeros(nb, bool), np.zeros(nb, bool)
    for ty, par, f, mu in entries:
        vi = np.zeros_like(p)
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            moved = moved.astype(bool)
        elif int(par[3]) == 0:
            q = p.copy()
            qs, sd, tri, cr = body.query_self(p[:nb], S["vid"], S["V"], *LENGTHS)
            mv = (sd > 0) & (tri >= 0)                                                  # (sdist = r - d > 0 or r + d: exactly the points the rule moves)
            assert np.array_equal(qs[~mv], p[:nb][~mv]) and not mv[S["vid"] < 0].any()
            q[:nb] = qs
            crossed |= cr.astype(bool); pushed |= mv & (cr == 0)
            pf, sdf = body.query(p[nb:])
            mf = sdf > 0
            q[nb:] = np.where(mf[:, None], pf, p[nb:])
            moved = np.concatenate([mv, mf])
            mu = mu_s
            if friction:
                vi[:nb], _, ids = body.velocity_query_self(p[:nb], S["vid"], S["V"], REACH, RHO, vel)
                assert (ids[mv] >= 0).all()
                vi[nb:] = pkg.mesh_velocity_query(body, None, p[nb:], vel)[0]
        elif int(par[3]) == 1:
            proj, sd = cube.query(p, par[:3], frame=f)
            moved = sd > 0
            q = np.where(moved[:, None], proj, p)
        else:
            q, sd, _, _ = shell.query_sided(p, sides, REACH_SHELL, par[:3])
            moved = (q != p).any(1)
        if friction and mu > 0:
            w = _np_rigid(np.zeros(9), q) + DT * vi
            q2, _ = pkg.friction_query_moving(p, q, x0, w, mu)
            q = np.where(moved[:, None], q2, q)
        p = q
    return p, crossed, pushed


def _kernel_system(pkg, entries, S, x0, self_collision, mu_s=0.0, shell=False, friction=True):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    n = len(x0)
    s.add_nodes(x0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    nb = len(S["x"])
    if self_collision is None:
        mid = s.add_body_surface(0, nb, S["F"])
    else:
        mid = s.add_body_surface(0, nb, S["F"], self_collision=self_collision)
    Vc, Fc = _cube()
    assert mid == 0 and s.add_collision_mesh(CUBE_S * Vc, Fc) == 1
    if shell:
        Vg, Fg = _grid()
        assert s.add_collision_mesh(pkg.Mesh(0.9 * Vg, Fg, R_SHELL), None) == 2
        s.set_collision_mesh_side_memory(2, REACH_SHELL)
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    s.set_collision_friction([e[3] if mu_s else 0.0 for e in entries])
    if mu_s:
        s.set_body_surface_friction(mid, mu_s)
    s.initialize()
    s.set_collision_frames([e[2] for e in entries])
    return s, b


@pytest.mark.gpu
@pytest.mark.parametrize("which,case", [(w, c) for w in ("short", "full") for c in ("plain", "surface_friction", "framed")] + [("shell", "plain")])
def test_bodyself_kernel_equals_host_composition(pkg, which, case):
    """the slotted bar (3, 3, 8) -- 144 nodes, 4 of them interior -- and 17 free particles, one collision element per node; the list
    [floor, the body itself, a closed cube], 64 entries of them, or the three and an open grid with side memory: z and u bitwise the
    host composition.  The body is registered open (its rest shape) and closed onto itself afterwards (the upper arm moved down by h
    with admm_hip_set_x); the surface the kernel meets is the device's frame-start update of it.  plain and framed: one local step of
    the batch alone on candidates xc + disp.  surface_friction: the body with a coefficient of its own, the nodes started with
    v = disp / dt, one frame of one iteration.  At least ten own nodes crossed and ten pushed on the outside; the interior nodes are
    not moved by the body's entry.  (The memory shell's list runs plain only: a step would latch its sides anew.)
    Measured on the MI355X: short list 21 own nodes crossed and 13 pushed on the outside, full list 23 to 24 and 16 to 23."""
    friction, framed = case == "surface_friction", case == "framed"
    S, x0, xc, disp = _kernel_scene(pkg)
    entries = _kernel_lists(framed, shell=True) if which == "shell" else _kernel_lists(framed)[which]
    nb = len(S["x"])
    mu_s = 0.5 if friction else 0.0
    rng = np.random.default_rng(173)
    u = np.where((rng.uniform(size=len(x0)) < 0.5)[:, None], 0.0005, 0.002) * rng.normal(size=x0.shape)
    body = pkg.Mesh(S["V"], S["Fl"])
    body.set_vertices(xc[S["sv"]])                                                      # (the arithmetic of the device's frame-start update)
    Vc, Fc = _cube()
    cube = pkg.Mesh(CUBE_S * Vc, Fc)
    s, b = _kernel_system(pkg, entries, S, x0, LENGTHS, mu_s, shell=which == "shell")
    assert s.collision_form() == 7
    s.m_x = xc.ravel()
    s.write_local(b, u=u)
    shell = sides = None
    if friction:
        v = disp / DT
        dx = xc + DT * v
        s.m_v = v.ravel()
        s.step(1)
    else:
        v = np.zeros_like(x0)
        dx = xc + disp
        if which == "shell":
            Vg, Fg = _grid()
            shell = pkg.Mesh(0.9 * Vg, Fg, R_SHELL)
            s.set_collision_sides(2, rng.integers(-1, 2, len(x0)).astype(np.int32))
        s.latch_collision_sides()                                                       # the launches a step begins with: the body's surface from the current x
        if which == "shell":
            sides = s.collision_sides(2)
            assert (sides != 0).sum() >= 10
        s.local_step_dx(b, dx)
    assert s.body_surface_status(0) == dict(updated=1, refused=0, last_bad_tri=-1)
    want, crossed, pushed = _kernel_compose(pkg, entries, S, body, cube, dx + u, xc, friction, mu_s, v[S["sv"]], shell, sides)
    r = s.read_local(b)
    print("%s list, %s: the body's entries: %d own nodes crossed, %d pushed on the outside" % (which, case, crossed.sum(), pushed.sum()))
    assert crossed.sum() >= 10 and pushed.sum() >= 10
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.flatnonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    # the interior nodes are unmoved by the body's entry: with the body's entries alone they keep their bits
    inner = np.flatnonzero(S["vid"] < 0)
    only = [e for e in entries if e[0] == MESH and int(e[1][3]) == 0]
    alone, _, _ = _kernel_compose(pkg, only, S, body, cube, dx + u, xc, friction, mu_s, v[S["sv"]])
    assert len(inner) == 4 and np.array_equal(alone[inner], (dx + u)[inner])
    if friction:
        still, _, _ = _kernel_compose(pkg, entries, S, body, cube, dx + u, xc, True, mu_s, np.zeros_like(v[S["sv"]]))
        assert np.abs(still - want).max() > 1e-4                                         # the vertices' velocities matter


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 5: off changes nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def _frames(s, frames, iters=10):
    out = []
    for _ in range(frames):
        s.step(iters)
        out.append((s.m_x.copy(), s.m_v.copy()))
    return out


@pytest.mark.gpu
def test_off_changes_nothing(pkg):
    """the kernel scene moving under its nodes' velocities for four frames: a context with r = 0 is bitwise a context built without the
    new call -- frames, collision_form 2 (a body surface with a coefficient), graph state; with self-collision on the form is 7 exactly
    while the list names the body, and a list that does not name it gives form 1 and the same bits whether the body self-collides or not"""
    S, x0, xc, disp = _kernel_scene(pkg)
    entries = _kernel_lists(False)["short"]
    res = {}
    for key in (None, (0.0, 0.0, 0.0), LENGTHS):
        s, _ = _kernel_system(pkg, entries, S, x0, key, mu_s=0.5)
        s.m_x = xc.ravel()
        s.m_v = (disp / DT).ravel()
        res[key] = (_frames(s, 4), s.collision_form(), s.graph_state())
    off = (0.0, 0.0, 0.0)
    assert res[None][1] == res[off][1] == 2 and res[LENGTHS][1] == 7
    assert _same_frames(res[None][0], res[off][0]) and res[None][2] == res[off][2], (res[None][2], res[off][2])
    assert res[None][2]["frame_graph_iters"] == 10
    assert not _same_frames(res[None][0], res[LENGTHS][0])
    bare = [e for e in entries if not (e[0] == MESH and e[1][3] == 0.0)]
    out = {}
    for key in (None, LENGTHS):
        s, _ = _kernel_system(pkg, bare, S, x0, key, mu_s=0.5)
        s.m_x = xc.ravel()
        s.m_v = (disp / DT).ravel()
        out[key] = (_frames(s, 4), s.collision_form(), s.graph_state())
    assert out[None][1] == out[LENGTHS][1] == 1
    assert _same_frames(out[None][0], out[LENGTHS][0]) and out[None][2] == out[LENGTHS][2]
    # the form follows the list, and a change of form drops the captured graphs
    s, _ = _kernel_system(pkg, bare, S, x0, LENGTHS, mu_s=0.5)
    _frames(s, 2)
    assert s.collision_form() == 1 and s.graph_state()["frame_graph_iters"] == 10
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    g = s.graph_state()
    assert s.collision_form() == 7 and not g["iter_graph"] and g["frame_graph_iters"] == 0, g
    s.set_collision_shapes([e[0] for e in bare], [e[1] for e in bare])
    assert s.collision_form() == 0                                                      # (a list of another length starts without coefficients)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 6 and 7: a body closing on itself; launch modes, shards, the class API
# ---------------------------------------------------------------------------------------------------------------------------------
K_TET = 1e5           # with G_ARM: in the control run the arm's tip passes the lower arm's top plane (the CPU oracle: lowest node 2.2 h below it) at |v_y| <= 1.0
G_ARM = 4.0
ARM = (2, 3, 8)


def _arm_scene(pkg):
    """slotted_bar(2, 3, 8, 2): -> (S, m, anchors, upper, bottom): the spine and the lower arm anchored, the upper arm free; bottom:
    the upper arm's nodes on its lower face (y = 2 h at rest)"""
    S = _surface(pkg, ARM)
    x = S["x"]
    upper = _upper(x)
    m = pkg.meshgen.lumped_tet_mass(x, S["tets"], 1000.0)
    return S, m, np.flatnonzero(~upper).astype(np.int32), upper, upper & (np.abs(x[:, 1] - 2 * H) < 1e-9)


def _arm_system(pkg, self_collision, all_nodes=False, rank=0, world=1, mode=None, mu=0.0):
    """gravity acts on every node and moves the upper arm alone (the rest is anchored); collision elements on the upper arm's nodes, or
    (all_nodes, what a CollisionForce of the class API does) on every node"""
    S, m, anch, upper, _ = _arm_scene(pkg)
    x = S["x"]
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], S["tets"], [K_TET])
    s.add_forces(KIND["ANCHOR"], anch, [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32) if all_nodes else np.flatnonzero(upper).astype(np.int32), [W])
    s.add_gravity([0.0, -G_ARM, 0.0])
    if world > 1:
        s.set_shard(rank, world)
        if mode:
            s.set_shard_mode(mode)
    s.mid = s.add_body_surface(0, len(x), S["F"], self_collision=self_collision)
    if mu:
        s.set_body_surface_friction(s.mid, mu)
    s.set_collision_shapes([MESH], [[0, 0, 0, s.mid]])
    return s


@pytest.mark.gpu
def test_body_closes_on_itself(pkg):
    """slotted_bar(2, 3, 8, 2) of linear-strain tets, the spine and the lower arm anchored, the upper arm falling under gravity onto the
    lower one, 40 frames of 20 iterations; only the upper arm's nodes carry collision elements.  Control (self-collision off): some
    upper-arm node crosses the lower arm's top plane y = h while the largest |v_y| stays below (R - r) / dt = 1.5, the condition on the
    reach.  With self-collision on no bottom node of the upper arm changes the sign of its height over that plane and no frame is
    refused.  The resting gap (the lowest bottom node's height over the plane in units of r) is printed, no bound asserted on it.
    Measured on the MI355X: control: lowest upper-arm node 2.1583 h below the plane, largest |v_y| 1.000; on: resting gap 0.9883 r,
    lowest ever 0.7910 r, largest |v_y| 0.837."""
    _, _, _, upper, bottom = _arm_scene(pkg)
    out = {}
    for on in (True, False):
        s = _arm_system(pkg, LENGTHS if on else None); s.initialize()
        ys, vmax = [], 0.0
        for _ in range(40):
            s.step(20)
            X, V = s.m_x.reshape(-1, 3), s.m_v.reshape(-1, 3)
            ys.append(X[:, 1].copy() - H)
            vmax = max(vmax, np.abs(V[upper, 1]).max())
        out[on] = (np.array(ys), vmax, s.body_surface_status(s.mid), s.collision_form())
    ys, vmax, st, form = out[True]
    yc, vc = out[False][0], out[False][1]
    print("closing arm: control: lowest upper-arm node %.4f h below the plane, largest |v_y| %.3f (limit (R - r) / dt = %.3f); on: largest |v_y| %.3f" %
          (-yc[:, upper].min() / H, vc, (REACH - R_GAP) / DT, vmax))
    print("closing arm: resting gap %.4f r (lowest bottom node after 40 frames), lowest ever %.4f r" % (ys[-1][bottom].min() / R_GAP, ys[:, bottom].min() / R_GAP))
    assert form == 7 and out[False][3] == 0
    assert (yc[:, upper] < 0).any() and vc < (REACH - R_GAP) / DT
    assert st == dict(updated=40, refused=0, last_bad_tri=-1) and out[False][2]["refused"] == 0
    assert (ys[:, bottom] > 0).all()


def _mode_results(pkg):
    s = _arm_system(pkg, LENGTHS, all_nodes=True, mu=0.3); s.initialize()
    fr = _frames(s, 12)
    return dict(x=np.array([f[0] for f in fr]), v=np.array([f[1] for f in fr]))


def _child_main(path):
    from __graft_entry__ import load_package
    np.savez(path, **_mode_results(load_package()))


@pytest.mark.gpu
def test_body_self_collision_launch_modes_bitwise(pkg, monkeypatch, tmp_path):
    """twelve frames of the closing arm (every node with a collision element, a surface coefficient; the arm reaches the lower one
    within them): eager, iteration graph, frame graph in this process and ADMM_HIP_LOCAL_MULTI=0 in a fresh child process give the same
    bits"""
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
    code = "import sys; sys.path[:0] = [%r, %r]; import test_body_self_collision as t; t._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.load(path)
    for name, v in res[keys[0]].items():
        assert np.array_equal(got[name], v), name
    # the self-collision acted within these frames: a control without it ends elsewhere
    c = _arm_system(pkg, None, all_nodes=True, mu=0.3); c.initialize()
    assert np.abs(_frames(c, 12)[-1][0] - res[keys[0]]["x"][-1]).max() > 1e-4


@pytest.mark.gpu
def test_body_self_collision_two_subtree_shards(pkg, monkeypatch):
    """the same twelve frames in two subtree shards (two contexts on one GPU): the ranks bitwise equal and within 1e-9 of one rank
    (measured on the MI355X: 2.5e-15)"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    ref = _arm_system(pkg, LENGTHS, all_nodes=True, mu=0.3); ref.initialize()
    refx = _frames(ref, 12)
    shards = [_arm_system(pkg, LENGTHS, all_nodes=True, rank=r, world=2, mode="subtree", mu=0.3) for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    assert all(s.collision_form() == 7 for s in shards)
    res, errs = [None, None], []

    def run(r):
        try:
            res[r] = _frames(shards[r], 12)
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    assert _same_frames(res[0], res[1])
    worst = max(np.abs(res[0][f][0] - refx[f][0]).max() for f in range(12))
    print("two subtree shards against one rank: |x - x_1| %.3g" % worst)
    assert worst < 1e-9, worst


def test_cpp_body_self_collision_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_body_self_collision", pkg))


@pytest.mark.gpu
def test_class_api_body_self_collision(pkg, tmp_path):
    """the closing arm through admm::System with CollisionBody::self_collision set: bitwise the C ABI's frames"""
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_body_self_collision", pkg)
    S, m, anch, _, _ = _arm_scene(pkg)
    x = S["x"]
    frames, iters = 12, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(S["tets"]), len(anch), len(S["F"])], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (S["tets"], anch, S["F"]):
            np.asarray(a).astype(np.int32).tofile(f)
        np.array([K_TET, G_ARM, DT, 0.3, *LENGTHS]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(outp).reshape(frames, 2, len(x) * 3)
    s = _arm_system(pkg, LENGTHS, all_nodes=True, mu=0.3); s.initialize()
    want = _frames(s, frames, iters)
    for f in range(frames):
        assert np.array_equal(got[f, 0], want[f][0]) and np.array_equal(got[f, 1], want[f][1]), (f, np.abs(got[f, 0] - want[f][0]).max())
