"""Side memory for thick shells (admm_hip_set_collision_mesh_side_memory; csrc/mesh_query.hpp: side_latch, sided_project): an open mesh with
a reach R >= r keeps one side per node, latched once per frame from the frame-start position, and a node that crosses the mid-surface
within a frame is mirrored back to distance r on the side it remembers.

CPU: the host rule against an np.longdouble reference (closest point by exhaustive search, side by the parity of the crossings of the
segment from a pole the surface is star-shaped from), a float64 restatement of the stated operation order, the reductions to the
existing rules, the latch table case by case, the refusals.  GPU: the latch kernel and the sided projection kernel against the host
routines bit for bit, a context without memory unchanged, particles that no longer tunnel, a swept sheet, a fast tet block, the launch
modes, two shards, a checkpoint with the sides."""
import os
import subprocess
import sys

import numpy as np
import pytest

from checkers import KIND
from test_collision_friction import DT, G, W, _expect, _kernel_case
from test_collision_frames import BOX, IDENT, _frame, _quarter, _rot, _rotate, _to_local, _to_world
from test_collision_mesh import FLOOR, MESH
from test_collision_shell import (N_NODES, _brute, _capped_icosphere, _cube, _drop_scene, _drop_system, _extent, _grid, _quarter_cylinder,
                                  _run, _same_frames)
from test_moving_friction import _np_rigid

L = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SHELL = 0.0625      # the half thickness r of the CPU tests' meshes
REACH = 0.25          # their reach R (both exactly representable)
BIG = 8.0             # the grid's pole lies this far below a point, along y


# ---------------------------------------------------------------------------------------------------------------------------------
# surfaces, each oriented so that its normals point away from a pole from which it is star-shaped
# ---------------------------------------------------------------------------------------------------------------------------------
def _surfaces():
    Vg, Fg = _grid()                                        # normals +y: away from a pole far below, rays along y
    Vc, Fc = _quarter_cylinder()
    Fc = np.ascontiguousarray(Fc[:, [0, 2, 1]])             # as built its normals point to the axis: flipped, away from it
    Vi, Fi = _capped_icosphere()                            # outward: away from the centre
    return {"grid": (Vg, Fg), "cylinder": (Vc, Fc), "capped_ico": (Vi, Fi)}


def _pole(name, P):
    """the pole of every point: below it for the grid, on the axis (x = 0, y = 2 / pi) at its z for the cylinder, the centre for the sphere"""
    P = np.asarray(P)
    o = np.zeros_like(P)
    if name == "grid":
        o[:, 0] = P[:, 0]; o[:, 1] = -BIG; o[:, 2] = P[:, 2]
    elif name == "cylinder":
        o[:, 1] = 2 / np.pi; o[:, 2] = P[:, 2]
    return o


def _seeded(V, F, R, seed, n=1500):
    """n points within 2 R of the surface -- at a uniform distance in (0, 2 R) from random points of it along the face normal, both sides
    -- and a seeded side in {-1, 0, 1} for each"""
    rng = np.random.default_rng(seed)
    f = F[rng.integers(0, len(F), n)]
    w = rng.dirichlet([1, 1, 1], n)
    base = (w[:, :, None] * V[f]).sum(1)
    nrm = np.cross(V[f[:, 1]] - V[f[:, 0]], V[f[:, 2]] - V[f[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    jit = rng.uniform(size=n) < 0.25                        # a quarter of them also moved sideways by up to R / 2 per axis: beside the rim
    dist = np.where(jit, rng.uniform(0, R, n), rng.uniform(0, 2 * R, n))
    P = base + (dist * np.where(rng.uniform(size=n) < 0.5, -1, 1))[:, None] * nrm + jit[:, None] * rng.uniform(-R / 2, R / 2, (n, 3))
    return np.ascontiguousarray(P), rng.integers(-1, 2, n).astype(np.int32)


def _boundary_edges(F):
    """the edges used by one triangle only, from the edge counts"""
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    u, cnt = np.unique(e, axis=0, return_counts=True)
    return u[cnt == 1]


def _dist_to_segments(c, A, B):
    """the distance of every point c [n][3] to the nearest of the segments (A_k, B_k), np.longdouble"""
    ab = (B - A)[None]
    t = ((c[:, None] - A[None]) * ab).sum(2) / (ab * ab).sum(2)
    t = np.clip(t, 0, 1)
    return np.sqrt(((A[None] + t[..., None] * ab - c[:, None]) ** 2).sum(2)).min(1)


def _ray_side(V, F, o, P, margin):
    """the side of every point by the crossings of the ray from its pole o through it, np.longdouble: +1 when the segment o -> P crosses
    the surface (an odd number of times: once, the surface being star-shaped from the pole), -1 when the ray crosses it beyond P, 0
    when the ray misses it -> (side, clear): clear is False where the ray passes an edge nearer than the margin"""
    V = V.astype(L); o = o.astype(L); P = P.astype(L)
    A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(B - A, C - A)                                                           # [nt][3], length = twice the area
    d = P - o
    den = d @ n.T                                                                        # [np][nt]
    num = ((A[None] - o[:, None]) * n[None]).sum(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = num / den
    X = o[:, None] + t[..., None] * d[:, None]                                           # the line's point in every triangle's plane
    n2 = (n * n).sum(1)

    def edge_dist(Pa, Pb, Pc):
        """the signed distance of X to the line (Pa, Pb) inside the triangle's plane, positive on Pc's side"""
        e = Pb - Pa
        inward = np.cross(n, e)                                                          # in the plane, towards Pc
        inward = inward / np.sqrt((inward * inward).sum(1))[:, None]
        return ((X - Pa[None]) * inward[None]).sum(2)

    m = np.minimum(np.minimum(edge_dist(A, B, C), edge_dist(B, C, A)), edge_dist(C, A, B))
    ahead = np.isfinite(t) & (t > 0)
    inside = ahead & (m > 0)
    clear = ~(ahead & (np.abs(m) <= margin)).any(1) & ~(np.abs(den) <= 1e-12 * np.sqrt(n2)[None] * np.sqrt((d * d).sum(1))[:, None]).any(1)
    seg = (inside & (t < 1)).sum(1)
    beyond = (inside & (t >= 1)).sum(1)
    side = np.where(seg % 2 == 1, 1, np.where(beyond > 0, -1, 0))
    return side, clear


_REF = {}


def _reference(name, seed):
    """the reference of one surface and seed, computed once, before the library is consulted: dict(P, s, c, d, boundary, side, clear, ext)"""
    key = (name, seed)
    if key not in _REF:
        V, F = _surfaces()[name]
        ext = _extent(V)
        P, s = _seeded(V, F, REACH, seed)
        c, d, tri = _brute(V, F, P)
        be = _boundary_edges(F)
        bd = _dist_to_segments(c, V[be[:, 0]].astype(L), V[be[:, 1]].astype(L))
        side, clear = _ray_side(V, F, _pole(name, P), P, 1e-9 * ext)
        for a in (P, s):
            a.setflags(write=False)
        _REF[key] = dict(V=V, F=F, P=P, s=s, c=c, d=d, tri=tri, boundary=bd <= 1e-9 * ext, side=side, clear=clear, ext=ext)
    return _REF[key]


SEEDS = {"grid": 101, "cylinder": 102, "capped_ico": 103}


def _expected(ref, s, r, R):
    """what the rule must decide for sides s on the reference's points -> (hit, known, crossed, moved, left_out): known = the side
    decision is the reference's to make (a hit that is no boundary hit, with the ray's side known); left_out = within a margin"""
    ext, d = ref["ext"], ref["d"]
    m = 1e-9 * ext
    hit = d < R
    out = np.abs(d - R) <= m
    sided = hit & ~ref["boundary"] & (s != 0)
    known = sided & (ref["side"] != 0)
    out |= known & (~ref["clear"] | (d <= m))
    crossed = known & (ref["side"] * s < 0)
    out |= hit & ~crossed & (np.abs(d - r) <= m)
    moved = crossed | (hit & (d < r))
    return hit, known, crossed, moved, out


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 1: the host rule against the np.longdouble reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid", "cylinder", "capped_ico"])
def test_host_rule_vs_longdouble(pkg, name):
    """1500 seeded points within 2 R of each surface with seeded sides.  Exact: hit or none within R, collides or not, crossed or not
    (outside the margins 1e-9 extent).  proj within 1e-12 (extent + |q|)(1 + r / d) of the reference's; a crossed point at distance r
    from the closest point to 1e-12 (extent + |q|).  Points whose ray misses the surface are evaluated with side 0, boundary hits must
    take the unsigned rule.  Measured, from the reference alone: left out by the margins (at most 1 %) grid 0.00 %, cylinder 0.00 %,
    capped icosphere 0.00 %; the ray misses for 2.6 %, 7.6 %, 2.6 % of the points; boundary hits within R 2.1 %, 3.2 %, 1.3 %."""
    r, R = R_SHELL, REACH
    ref = _reference(name, SEEDS[name])
    P, c, d, ext = ref["P"], ref["c"], ref["d"], ref["ext"]
    miss = (ref["side"] == 0) & ~ref["boundary"]
    s = np.where(miss, 0, ref["s"]).astype(np.int32)                                   # the ray misses: the unsigned rule only
    hit, known, crossed, moved, out = _expected(ref, s, r, R)
    share = out.mean()
    print("%s: left out by the margins %.2f %%, ray misses %.1f %%, boundary hits %.1f %%, crossed %d, pushed on their side %d"
          % (name, 100 * share, 100 * (ref["side"] == 0).mean(), 100 * (ref["boundary"] & hit).mean(), int(crossed.sum()), int((moved & ~crossed).sum())))
    assert share <= 0.01, share
    assert crossed.sum() >= 100 and (moved & ~crossed).sum() >= 100 and (ref["boundary"] & hit & (ref["s"] != 0)).sum() >= 10
    m = pkg.Mesh(ref["V"], ref["F"], r)
    proj, sd, tri, cr = m.query_sided(P, s, R)
    keep = ~out
    got_moved = (proj != P).any(1)
    assert np.array_equal(m.side_latch(P, 1, R)[keep & ~ref["boundary"]] != 0, hit[keep & ~ref["boundary"]])      # hit or none within R
    assert np.array_equal(got_moved[keep], moved[keep])
    assert np.array_equal(cr[keep] != 0, crossed[keep])
    assert not cr[ref["boundary"] & keep].any()
    k = keep & moved
    e = (P.astype(L) - c)[k]
    sc = (r / d[k])[:, None]
    want = np.where(crossed[k][:, None], c[k] - sc * e, c[k] + sc * e)
    bound = 1e-12 * (ext + np.linalg.norm(P[k], axis=1)) * (1 + r / d[k].astype(np.float64))
    err = np.linalg.norm((proj[k].astype(L) - want).astype(np.float64), axis=1)
    assert (err <= bound).all(), (err / bound).max()
    kc = keep & crossed
    off = np.abs(np.linalg.norm((proj[kc].astype(L) - c[kc]).astype(np.float64), axis=1) - r)
    assert (off <= 1e-12 * (ext + np.linalg.norm(P[kc], axis=1))).all(), off.max()
    assert np.array_equal(sd[keep & ~moved], np.full(int((keep & ~moved).sum()), -np.inf))
    assert (sd[kc] > r).all() and (sd[keep & moved & ~crossed] > 0).all() and (sd[keep & moved & ~crossed] <= r).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 2: the stated operation order in float64 numpy, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
def _restate_sided(m, P, s, r, R, t, f=None):
    """mesh_query.hpp's projection in plain float64 numpy on the library's own hits (Mesh.closest bounded by R * R or r * r) and stored
    pseudo-normals (Mesh.feature_normal) -> (proj, sdist, crossed)"""
    t = np.asarray(t, dtype=np.float64)
    framed = f is not None and not np.array_equal(np.asarray(f)[:9], IDENT[:9])
    q = (_to_local(f, P) if framed else P) - t
    inf = m.info()
    bits, _ = m.boundary_table()
    proj, sd, cr = P.copy(), np.full(len(P), -np.inf), np.zeros(len(P), np.int32)
    hR, hr = m.closest(q, R * R), m.closest(q, r * r)
    for i in range(len(P)):
        h = hR if s[i] != 0 else hr
        rad = R if s[i] != 0 else r
        if not ((inf["lo"] - rad < q[i]) & (q[i] < inf["hi"] + rad)).all() or h["slot"][i] < 0:
            continue
        c, d2 = h["c"][i], h["d2"][i]
        e = q[i] - c
        crossed = False
        if s[i] != 0:
            n = m.feature_normal(h["slot"][i:i + 1], h["reg"][i:i + 1])[0]
            g = (q[i, 0] - c[0]) * n[0] + (q[i, 1] - c[1]) * n[1] + (q[i, 2] - c[2]) * n[2]
            so = 1 if g > 0 else (-1 if g < 0 else 0)
            boundary = (bits[h["slot"][i]] >> h["reg"][i]) & 1
            crossed = not (boundary or so * s[i] >= 0 or not d2 > 0)
        d = np.sqrt(d2)
        if crossed:
            sc = r / d
            o = c - sc * e
            sd[i] = r + d
        else:
            if not d2 < r * r:
                continue
            o = c + (r / d) * e if d > 0 else c + r * m.feature_normal(h["slot"][i:i + 1], [0])[0]
            sd[i] = r - d
        cr[i] = crossed
        l = (t + o)[None]
        proj[i] = (_to_world(f, l) if framed else l)[0]
    return proj, sd, cr


@pytest.mark.parametrize("name", ["grid", "cylinder", "capped_ico"])
def test_float64_restatement_is_bitwise(pkg, name):
    """g, the boundary bit, the mirror push, the translation and the frame, restated in float64 numpy on the points of test 1 (moved and
    turned along with the instance): proj, sdist and crossed of query_sided bit for bit"""
    r, R = R_SHELL, REACH
    ref = _reference(name, SEEDS[name])
    m = pkg.Mesh(ref["V"], ref["F"], r)
    t = np.array([0.375, -0.125, 0.25])
    f = _frame(_rot([0.3, -1.0, 0.5], 0.7), [0.1, 0.2, -0.3])
    for frame in (None, f):
        P = ref["P"] + t
        if frame is not None:
            P = _to_world(frame, P)
        proj, sd, tri, cr = m.query_sided(P, ref["s"], R, t, frame)
        wp, wsd, wcr = _restate_sided(m, P, ref["s"], r, R, t, frame)
        assert cr.sum() >= 100 and ((proj != P).any(1) & (cr == 0)).sum() >= 50
        assert np.array_equal(proj, wp) and np.array_equal(sd, wsd) and np.array_equal(cr, wcr)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 3: reductions to the existing rules
# ---------------------------------------------------------------------------------------------------------------------------------
def test_reductions(pkg):
    r, R = R_SHELL, REACH
    t = np.array([0.375, -0.125, 0.25])
    f = _frame(_rot([0.3, -1.0, 0.5], 0.7), [0.1, 0.2, -0.3])
    for name in ("grid", "cylinder", "capped_ico"):
        ref = _reference(name, SEEDS[name])
        m = pkg.Mesh(ref["V"], ref["F"], r)
        for frame in (None, f):                                                      # side all zero: Mesh.query, bitwise
            P = ref["P"] + t if frame is None else _to_world(frame, ref["P"] + t)
            proj, sd, tri, cr = m.query_sided(P, 0, R, t, frame)
            wp, wsd = m.query(P, t, frame=frame)
            assert np.array_equal(proj, wp) and np.array_equal(sd, wsd) and not cr.any() and (sd > 0).sum() >= 100
    # a crossed point over a face of the flat grid lands exactly at (x, s r, z): coordinates with few bits, so every product is exact
    g = pkg.Mesh(*_grid(), r)
    k = np.arange(12)
    x = -0.5 + 3 / 64 + (k % 4) * 0.25 + (k // 4) / 64.0
    z = -0.5 + 1 / 64 + ((k * 5) % 4) * 0.25
    for s in (1, -1):
        for depth in (r / 2, 2 * r, 3 * r):
            P = np.stack([x, np.full(12, -s * depth), z], 1)
            proj, sd, tri, cr = g.query_sided(P, s, R)
            assert cr.all() and np.array_equal(proj, np.stack([x, np.full(12, s * r), z], 1)) and np.array_equal(sd, np.full(12, r + depth))
            same, sds, _, crs = g.query_sided(P * [1, -1, 1], s, R)                  # on its own side: pushed only from inside the shell
            assert not crs.any() and np.array_equal(same, np.stack([x, np.full(12, s * max(depth, r)), z], 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 4: the latch table
# ---------------------------------------------------------------------------------------------------------------------------------
def _latch_cases(R=REACH, r=R_SHELL):
    """points in the grid's own coordinates with the previous side and the side the latch must give, by case"""
    e = 1 / 64
    cases = {
        "outside_box": ([[0.5 + R, 0.0, 0.0], [0.0, R, 0.0], [0.0, -R - e, 0.125], [-0.5 - R - e, 0.0, 0.0], [0.0, 0.0, 0.5 + R]], [1, -1, 0, 1, -1], [0, 0, 0, 0, 0]),
        "beyond_reach": ([[0.5 + 0.75 * R, 0.75 * R, 0.0], [-0.5 - 0.75 * R, -0.75 * R, 0.125], [0.0, 0.75 * R, 0.5 + 0.75 * R],
                          [0.5 + 0.75 * R, 0.0, 0.5 + 0.75 * R], [0.5 + 0.75 * R, -0.75 * R, -0.25]], [1, -1, 0, 1, -1], [0, 0, 0, 0, 0]),
        "boundary_hit": ([[0.5 + e, 2 * r, 0.125], [0.5 + e, -2 * r, 0.125], [0.125, 2 * r, -0.5 - e], [0.5 + e, 0.125, 0.5 + e], [-0.5 - e, -0.125, 0.3125],
                          [0.5, 0.125, 0.125]], [1, -1, 1, -1, 1, 1], [0, 0, 0, 0, 0, 0]),
        "sticky": ([[0.125, -2 * r, 0.0625], [0.125, 2 * r, 0.0625], [0.3125, -r / 2, -0.1875], [0.3125, r / 2, -0.1875], [0.0, -0.1875, 0.0], [0.25, 0.125, 0.25]],
                   [1, -1, 1, -1, 1, -1], [1, -1, 1, -1, 1, -1]),
        "learn_above": ([[0.125, 2 * r, 0.0625], [0.3125, r, -0.1875], [0.0, 0.1875, 0.0], [0.25, 0.125, 0.25], [-0.375, 0.234375, 0.4375]], [0] * 5, [1] * 5),
        "learn_below": ([[0.125, -2 * r, 0.0625], [0.3125, -r, -0.1875], [0.0, -0.1875, 0.0], [0.25, -0.125, 0.25], [-0.375, -0.234375, 0.4375]], [0] * 5, [-1] * 5),
        "inside_shell": ([[0.125, r / 2, 0.0625], [0.3125, -r / 2, -0.1875], [0.0, r - e / 4, 0.0], [0.25, -r + e / 4, 0.25], [-0.375, e, 0.4375]], [0] * 5, [0] * 5),
        "g_zero": ([[0.125, 0.0, 0.0625], [0.25, 0.0, 0.25], [0.0, 0.0, 0.0], [0.5 + 2 * r, 0.0, 0.125], [0.125, 0.0, -0.5 - 3 * r]], [0] * 5, [0] * 5),
    }
    return {k: (np.array(p, dtype=np.float64), np.array(s, dtype=np.int32), np.array(w, dtype=np.int32)) for k, (p, s, w) in cases.items()}


def _latch_case_of(m, q, prev, r, R):
    """the case of the latch table every point falls under, from the library's own search (names as in _latch_cases; learn = 0 with
    g == 0 counts as g_zero, as does a point on the surface)"""
    inf = m.info()
    box = ((inf["lo"] - R < q) & (q < inf["hi"] + R)).all(1)
    h = m.closest(q, R * R)
    bits, _ = m.boundary_table()
    out = []
    for i in range(len(q)):
        if not box[i]:
            out.append("outside_box"); continue
        if h["slot"][i] < 0:
            out.append("beyond_reach"); continue
        n = m.feature_normal(h["slot"][i:i + 1], h["reg"][i:i + 1])[0]
        c = h["c"][i]
        g = (q[i, 0] - c[0]) * n[0] + (q[i, 1] - c[1]) * n[1] + (q[i, 2] - c[2]) * n[2]
        if (bits[h["slot"][i]] >> h["reg"][i]) & 1:
            out.append("boundary_hit" if prev[i] != 0 else ("g_zero" if g == 0 else "boundary_unset"))
        elif prev[i] != 0:
            out.append("sticky" if g * prev[i] < 0 else "kept")
        elif g == 0:
            out.append("g_zero")
        elif h["d2"][i] < r * r:
            out.append("inside_shell")
        else:
            out.append("learn_above" if g > 0 else "learn_below")
    return np.array(out)


def test_latch_table_case_by_case(pkg):
    r, R = R_SHELL, REACH
    g = pkg.Mesh(*_grid(), r)
    t = np.array([0.25, -0.5, 0.125])
    f = _frame(_quarter(0, 1), [0.5, 0.25, -0.25])                                    # an exact quarter turn: the cases stay exact
    for name, (q, prev, want) in _latch_cases().items():
        assert np.array_equal(g.side_latch(q, prev, R), want), name
        assert np.array_equal(g.side_latch(_to_world(f, q + t), prev, R, t, f), want), name
        kinds = _latch_case_of(g, q, prev, r, R)
        assert (kinds == name).all(), (name, kinds)


@pytest.mark.parametrize("name", ["grid", "cylinder", "capped_ico"])
def test_latch_vs_longdouble(pkg, name):
    """the latch on 1500 seeded points per surface against the reference of test 1 under the same margins and cap: no hit within R or a
    boundary hit gives 0, a side is kept, side 0 learns the ray's side from d >= r on.  Left out (the margins, and points that would
    learn a side where the ray misses the surface), measured from the reference alone: grid 0.00 %, cylinder 0.67 %, capped icosphere
    0.27 %."""
    r, R = R_SHELL, REACH
    ref = _reference(name, SEEDS[name] + 10)
    s, d, m9 = ref["s"], ref["d"], 1e-9 * ref["ext"]
    hit = d < R
    free = hit & ~ref["boundary"]
    learn = free & (s == 0)
    out = (np.abs(d - R) <= m9) | (learn & ((np.abs(d - r) <= m9) | ((d >= r) & ((ref["side"] == 0) | ~ref["clear"]))))
    print("%s latch: left out %.2f %%, of them the ray misses %.2f %%" % (name, 100 * out.mean(), 100 * (learn & (d >= r) & (ref["side"] == 0)).mean()))
    assert out.mean() <= 0.01, out.mean()
    want = np.where(free, np.where(s != 0, s, np.where(d >= r, ref["side"], 0)), 0)
    got = pkg.Mesh(ref["V"], ref["F"], r).side_latch(ref["P"], s, R)
    assert np.array_equal(got[~out], want[~out])
    assert (want[~out & learn] == 1).sum() >= 50 and (want[~out & learn] == -1).sum() >= 50 and (~out & learn & (d < r)).sum() >= 20


def test_boundary_table(pkg):
    """bit reg of a slot is set exactly for its boundary edges (used by one triangle) and the vertices on one, in the slot's rotated
    corner order; a closed mesh has none"""
    for name, (V, F) in _surfaces().items():
        m = pkg.Mesh(V, F, R_SHELL)
        bits, orig = m.boundary_table()
        be = {tuple(e) for e in _boundary_edges(F)}
        bv = {v for e in be for v in e}
        assert sorted(orig) == list(range(len(F))) and len(be) > 0
        for b, t in zip(bits, orig):
            T = [int(v) for v in F[t]]
            k0 = int(np.argmin(T))
            T = T[k0:] + T[:k0]
            want = 0
            for k in range(3):
                if tuple(sorted((T[k], T[(k + 1) % 3]))) in be:
                    want |= 1 << (1 + k)
                if T[k] in bv:
                    want |= 1 << (4 + k)
            assert b == want, (name, t, b, want)
    Vc, Fc = _cube()
    assert not pkg.Mesh(Vc, Fc, R_SHELL).boundary_table()[0].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 5: refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_side_memory_refusals(pkg):
    x = np.random.default_rng(0).uniform(-1, 1, size=(12, 3))
    s = pkg.System(device_id=-1)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    og = s.add_collision_mesh(pkg.Mesh(*_grid(), R_SHELL), None)
    Vc, Fc = _cube()
    cc = s.add_collision_mesh(Vc, Fc)
    o2 = s.add_collision_mesh(pkg.Mesh(*_quarter_cylinder(), R_SHELL), None)
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(cc, 0.5), "error 1", "mesh %d" % cc, "closed")
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(og, R_SHELL / 2), "error 1", "mesh %d" % og, "below its half thickness")
    for bad in (np.inf, -np.inf, np.nan):
        _expect(pkg, lambda: s.set_collision_mesh_side_memory(og, bad), "error 1", "mesh %d" % og, "not finite")
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(-1, 0.5), "error 1", "mesh_id -1")
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(7, 0.5), "error 1", "mesh_id 7")
    assert s.collision_form() == 0
    s.set_collision_shapes([MESH, FLOOR], [[0, 0, 0, og], [0, -1, 0, 0]])
    assert s.collision_form() == 4
    s.set_collision_mesh_side_memory(og, 0.5)
    assert s.collision_form() == 6
    s.set_collision_mesh_side_memory(og, 0.0)                                          # off again
    assert s.collision_form() == 4
    s.set_collision_mesh_side_memory(og, R_SHELL)                                      # R == r is allowed
    s.set_collision_mesh_side_memory(og, 0.5)
    _expect(pkg, lambda: s.set_collision_mesh_thickness(og, 0.75), "error 1", "mesh %d" % og, "exceeds the reach")
    s.set_collision_mesh_thickness(og, 0.125)
    s.set_collision_mesh_thickness(o2, 0.75)                                           # a mesh without memory: no such bound
    _expect(pkg, lambda: s.set_collision_shapes([MESH, FLOOR, MESH], [[0, 0, 0, og], [0, -1, 0, 0], [1, 0, 0, og]]), "error 1", "shapes 0 and 2", "mesh %d" % og)
    s.set_collision_shapes([MESH, MESH, MESH], [[0, 0, 0, o2], [1, 0, 0, o2], [0, 0, 0, og]])      # a mesh without memory may be named twice
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(o2, 1.0), "error 1", "shapes 0 and 1", "mesh %d" % o2)
    _expect(pkg, lambda: s.collision_sides(og), "error 3")                             # the sides exist from initialize on
    s.initialize()
    _expect(pkg, lambda: s.set_collision_mesh_side_memory(og, 0.5), "error 3", "before finalize")
    _expect(pkg, lambda: s.set_collision_mesh_thickness(og, 0.75), "error 1", "exceeds the reach")
    _expect(pkg, lambda: s.set_collision_shapes([MESH, MESH], [[0, 0, 0, og], [1, 0, 0, og]]), "error 1", "shapes 0 and 1")
    assert np.array_equal(s.collision_sides(og), np.zeros(12, np.int32))
    side = np.array([1, -1, 0] * 4, dtype=np.int32)
    s.set_collision_sides(og, side)
    assert np.array_equal(s.collision_sides(og), side)
    for bad in (2, -2, 7):
        _expect(pkg, lambda: s.set_collision_sides(og, np.where(np.arange(12) == 5, bad, side)), "error 1", "node 5", "-1, 0 or 1")
    assert np.array_equal(s.collision_sides(og), side)
    for wrong in (-1, 9):
        _expect(pkg, lambda: s.collision_sides(wrong), "error 1", "mesh_id %d" % wrong)
        _expect(pkg, lambda: s.set_collision_sides(wrong, side), "error 1", "mesh_id %d" % wrong)
    _expect(pkg, lambda: s.collision_sides(o2), "error 1", "mesh %d" % o2, "no side memory")
    _expect(pkg, lambda: s.collision_sides(cc), "error 1", "no side memory")
    _expect(pkg, lambda: s.set_collision_sides(og, side[:5]), "5 sides given")
    s.reset_collision_sides()
    assert not s.collision_sides(og).any()
    m = pkg.Mesh(*_grid(), R_SHELL)
    P = np.zeros((3, 3))
    for call in (lambda: m.side_latch(P, 0, R_SHELL / 2), lambda: m.side_latch(P, 0, np.inf), lambda: m.side_latch(P, 2, 0.5),
                 lambda: m.query_sided(P, 0, R_SHELL / 2), lambda: m.query_sided(P, 0, np.nan), lambda: m.query_sided(P, -3, 0.5),
                 lambda: pkg.Mesh(Vc, Fc).side_latch(P, 0, 0.5), lambda: pkg.Mesh(Vc, Fc).query_sided(P, 0, 0.5)):
        _expect(pkg, call, "error 1")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 7: the latch kernel equals the host latch
# ---------------------------------------------------------------------------------------------------------------------------------
N_LATCH = 130         # two 64-lane blocks and a partial one
LATCH_T = np.array([0.25, -0.5, 0.125])                                               # the grid entry's translation (exact)
LATCH_F = _frame(_quarter(0, 1), [0.5, 0.25, -0.25])                                  # ... and frame: an exact quarter turn about x
CYL_T = np.array([-0.4, 0.3, 0.6])


def _latch_scene():
    """-> (x [130][3], prev sides of the grid and of the cylinder): the 46 points of the latch table placed exactly in the framed grid's
    coordinates with their previous sides, the rest seeded around both memory meshes"""
    rng = np.random.default_rng(131)
    cases = _latch_cases()
    q = np.concatenate([c[0] for c in cases.values()]); pg = np.concatenate([c[1] for c in cases.values()])
    x = np.zeros((N_LATCH, 3)); sg = rng.integers(-1, 2, N_LATCH).astype(np.int32)
    x[:len(q)] = _to_world(LATCH_F, q + LATCH_T); sg[:len(q)] = pg
    rest = N_LATCH - len(q)
    Vg, Fg = _grid(); Vc, Fc = _quarter_cylinder()
    a = _seeded(Vg, Fg, REACH, 132, rest // 2)[0]
    b = _seeded(Vc, Fc, REACH, 133, rest - rest // 2)[0]
    x[len(q):] = np.concatenate([_to_world(LATCH_F, a + LATCH_T), b + CYL_T])
    return x, sg, rng.integers(-1, 2, N_LATCH).astype(np.int32)


def _latch_system(pkg, x):
    Vc, Fc = _cube()
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.ones(x.size))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.grid = s.add_collision_mesh(pkg.Mesh(*_grid(), R_SHELL), None)
    s.cyl = s.add_collision_mesh(pkg.Mesh(*_quarter_cylinder(), R_SHELL), None)
    s.cube = s.add_collision_mesh(0.6 * Vc, Fc)
    s.ico = s.add_collision_mesh(pkg.Mesh(*_capped_icosphere(), R_SHELL), None)
    s.set_collision_mesh_side_memory(s.grid, REACH)
    s.set_collision_mesh_side_memory(s.cyl, REACH)
    s.set_collision_shapes([FLOOR, MESH, MESH, MESH, MESH],
                           [[0, -2.0, 0, 0], [*LATCH_T, s.grid], [*CYL_T, s.cyl], [0.1, 0.2, 0.3, s.cube], [-0.3, 0.1, 0.2, s.ico]])
    s.initialize()
    s.set_collision_frames([IDENT, LATCH_F, IDENT, IDENT, IDENT])
    return s


def test_latch_scene_counts(pkg):
    """the seeds of the GPU latch test, checked on the host: every case of the latch table occurs at least five times among the 130 nodes"""
    x, sg, _ = _latch_scene()
    g = pkg.Mesh(*_grid(), R_SHELL)
    kinds = _latch_case_of(g, _to_local(LATCH_F, x) - LATCH_T, sg, R_SHELL, REACH)
    for name in _latch_cases():
        assert (kinds == name).sum() >= 5, (name, int((kinds == name).sum()))


@pytest.mark.gpu
def test_latch_kernel_equals_host_latch(pkg):
    """130 nodes, the list [floor, a framed memory grid, a translated memory quarter cylinder, a closed cube, an open mesh without
    memory]: seeded previous sides through set_collision_sides, then latch_collision_sides three times with x moved in between -- the
    sides of both memory meshes equal Mesh.side_latch exactly, every time"""
    x, sg, sc = _latch_scene()
    s = _latch_system(pkg, x)
    assert s.collision_form() == 6
    g, c = pkg.Mesh(*_grid(), R_SHELL), pkg.Mesh(*_quarter_cylinder(), R_SHELL)
    _expect(pkg, lambda: s.collision_sides(s.ico), "error 1", "no side memory")
    s.set_collision_sides(s.grid, sg); s.set_collision_sides(s.cyl, sc)
    rng = np.random.default_rng(134)
    for k in range(3):
        s.latch_collision_sides()
        wg, wc = g.side_latch(x, sg, REACH, LATCH_T, LATCH_F), c.side_latch(x, sc, REACH, CYL_T)
        gg, gc = s.collision_sides(s.grid), s.collision_sides(s.cyl)
        print("latch %d: grid sides -1 / 0 / 1: %s, cylinder: %s; changed %d, %d" % (k, [int((wg == v).sum()) for v in (-1, 0, 1)], [int((wc == v).sum()) for v in (-1, 0, 1)],
                                                                                    int((wg != sg).sum()), int((wc != sc).sum())))
        assert np.array_equal(gg, wg) and np.array_equal(gc, wc), k
        assert (wg != sg).sum() >= 5
        sg, sc = wg, wc
        x = x + rng.uniform(-0.12, 0.12, x.shape)
        s.m_x = x.ravel()
    s.reset_collision_sides()
    assert not s.collision_sides(s.grid).any() and not s.collision_sides(s.cyl).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 8: the sided kernel equals the host composition
# ---------------------------------------------------------------------------------------------------------------------------------
R_K = 0.125           # the half thickness of the kernel test's open meshes
REACH_K = 0.375
GRID_TK = np.array([0.125, -0.25, 0.0])
ICO_TK = np.array([-0.2, 0.15, 0.1])
MOTION_K = np.array([0.4, 0.2, -0.3, 1.0, 2.0, -1.5, 0.5, 0.2, 0.1])


def _sided_meshes():
    """registered in this order: 0 the open grid (memory), 1 the closed cube, 2 the capped icosphere (memory), 3 the grid again (no memory)"""
    Vc, Fc = _cube()
    return [(*_grid(), R_K), (0.6 * Vc, Fc, None), (*_capped_icosphere(), R_K), (*_grid(), R_K)]


def _ico_vel(V):
    return np.stack([0.6 * np.sin(3 * V[:, 1]) + 0.4 * V[:, 2], -0.5 * V[:, 0] * V[:, 2] + 0.2, 0.7 * np.cos(2 * V[:, 0])], 1)      # not rigid


def _sided_lists():
    """entries (type, params, frame, mu, motion): floor, the memory grid with a rigid motion, the closed cube, a framed box, the memory
    icosphere under a frame; and 64 entries: those five, then floors, cubes, boxes and the grid without memory at seeded places"""
    rng = np.random.default_rng(141)
    z9 = np.zeros(9)
    f_ico = _frame(_rot(rng.normal(size=3), 0.9), ICO_TK + [0.05, -0.1, 0.0])
    short = [(FLOOR, [0.0, -0.42, 0.0, 0.0], IDENT.copy(), 0.3, z9),
             (MESH, [*GRID_TK, 0.0], IDENT.copy(), 0.5, MOTION_K),
             (MESH, [-0.3, 0.25, 0.3, 1.0], IDENT.copy(), 0.0, z9),
             (BOX, [0.4, 0.3, 0.4, 0.0], _frame(_rot([0.2, 0.1, 1.0], 0.6), [0.3, 0.35, -0.25]), np.inf, z9),
             (MESH, [*ICO_TK, 2.0], f_ico, 0.7, z9)]
    full = list(short)
    for k in range(5, 64):
        d = rng.uniform(-0.25, 0.25, 3)
        mu = [0.3, 0.0, 0.7, np.inf, 0.15][k % 5]
        kind = k % 4
        if kind == 0:
            full.append((FLOOR, [0.0, -0.42 + 0.1 * d[1], 0.0, 0.0], IDENT.copy(), mu, z9))
        elif kind == 1:
            full.append((MESH, [*(np.array([-0.3, 0.25, 0.3]) + d), 1.0], IDENT.copy(), mu, z9))
        elif kind == 2:
            full.append((BOX, [0.4, 0.3, 0.4, 0.0], _frame(_rot([0.2, 0.1, 1.0], 0.6), np.array([0.3, 0.35, -0.25]) + d), mu, z9))
        else:
            full.append((MESH, [*(np.array([0.0, 0.3, 0.0]) + d), 3.0], _frame(_rot(d, 0.4), d), mu, z9))
    return {"short": short, "full": full}


def _sided_case():
    """65 candidates p = dx + u, frame starts x0 and the sides of the two memory meshes: 16 over the grid on the wrong side within the
    reach (crossed), 16 over it inside the shell on their own side, 8 beside its rim inside the shell with a side set (boundary hits), the
    rest seeded, with seeded sides on the icosphere"""
    dx, x0, u = _kernel_case(N_NODES, 5)
    dx, x0, u = 0.6 * dx, 0.6 * x0, 0.6 * u
    rng = np.random.default_rng(142)
    p = dx + u
    sg = rng.integers(-1, 2, N_NODES).astype(np.int32); si = rng.integers(-1, 2, N_NODES).astype(np.int32)
    k = np.arange(16)
    p[k] = np.stack([rng.uniform(-0.45, 0.45, 16), rng.uniform(0.02, 0.9 * REACH_K, 16) * np.where(k % 2, 1, -1), rng.uniform(-0.45, 0.45, 16)], 1) + GRID_TK
    sg[k] = np.where(k % 2, -1, 1)
    k = np.arange(16, 32)
    p[k] = np.stack([rng.uniform(-0.45, 0.45, 16), rng.uniform(0.01, 0.95 * R_K, 16) * np.where(k % 2, 1, -1), rng.uniform(-0.45, 0.45, 16)], 1) + GRID_TK
    sg[k] = np.where(k % 2, 1, -1)
    k = np.arange(32, 40)
    p[k] = np.stack([0.5 + rng.uniform(0.01, 0.6 * R_K, 8), rng.uniform(-0.6 * R_K, 0.6 * R_K, 8), rng.uniform(-0.45, 0.45, 8)], 1) + GRID_TK
    sg[k] = np.where(k % 2, 1, -1)
    dx[:40] = p[:40] - u[:40]
    x0[:40] = p[:40] + 0.03 * rng.normal(size=(40, 3))
    return dx, x0, u, sg, si


def _sided_compose(pkg, entries, p, x0, sides, friction, moving):
    """the list's entries in order on the host: shape_query, Mesh.query (framed) or, for a mesh with memory, Mesh.query_sided with the
    installed sides, then the friction rule on the world-space points -> (z, counts: crossed, pushed on their own side with a side set,
    boundary hits with a side set)"""
    specs = _sided_meshes()
    meshes = [pkg.Mesh(V, F, r) for V, F, r in specs]
    bits = {mi: meshes[mi].boundary_table()[0] for mi in sides}
    crossed = np.zeros(len(p), bool); own = np.zeros(len(p), bool); bnd = np.zeros(len(p), bool)
    for ty, par, f, mu, motion in entries:
        vi = None
        if ty != MESH:
            q, moved = pkg.shape_query(ty, par, p, f)
            moved = moved.astype(bool)
        else:
            mi = int(par[3])
            framed = not np.array_equal(f[:9], IDENT[:9])
            loc = _to_local(f, p) if framed else p
            if mi in sides:
                proj, sd, tri, cr = meshes[mi].query_sided(p, sides[mi], REACH_K, par[:3], f)
                moved = sd > -np.inf
                h = meshes[mi].closest(loc - np.asarray(par[:3]), REACH_K ** 2)
                isb = (h["slot"] >= 0) & (((bits[mi][np.maximum(h["slot"], 0)] >> h["reg"]) & 1) != 0)
                crossed |= cr != 0
                own |= moved & (cr == 0) & (sides[mi] != 0) & ~isb
                bnd |= isb & (sides[mi] != 0)
            else:
                proj, sd = meshes[mi].query(p, par[:3], frame=f)
                moved = (proj != p).any(1) if specs[mi][2] else sd > 0
            q = np.where(moved[:, None], proj, p)
            if moving and mi == 2:                                                  # the icosphere's vertex velocities at the hit, turned by R
                vi, _, _ = pkg.mesh_velocity_query(meshes[mi], None, loc, _ico_vel(specs[2][0]), par[:3])
                if framed:
                    vi = _rotate(f, vi)
        if friction:
            w = _np_rigid(motion if moving else np.zeros(9), q)
            if vi is not None:
                w = w + DT * vi
            q2, mode = (pkg.friction_query_moving(p, q, x0, w, mu) if moving else pkg.friction_query(p, q, x0, mu))
            q = q2
        p = q
    return p, (int(crossed.sum()), int(own.sum()), int(bnd.sum()))


def _sided_system(pkg, entries, x0, friction, moving):
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    n = len(x0)
    s.add_nodes(x0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    for V, F, r in _sided_meshes():
        s.add_collision_mesh(pkg.Mesh(V, F, r), None)
    s.set_collision_mesh_side_memory(0, REACH_K); s.set_collision_mesh_side_memory(2, REACH_K)
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    s.set_collision_friction([e[3] if friction else 0.0 for e in entries])
    s.initialize()
    s.set_collision_frames([e[2] for e in entries])
    if moving:
        s.set_collision_motion([e[4] for e in entries])
        s.set_collision_mesh_velocity(2, _ico_vel(_sided_meshes()[2][0]))
    return s, b


def test_sided_case_counts(pkg):
    """the seeds of the GPU kernel test, checked on the host: at least a fifth of the 65 nodes are crossed, at least a fifth are pushed on
    their own side, at least three hit a boundary feature with a side set -- in both lists, with and without friction"""
    dx, x0, u, sg, si = _sided_case()
    for which, entries in _sided_lists().items():
        assert len(entries) == (5 if which == "short" else 64)
        for friction, moving in ((False, False), (True, False), (True, True)):
            _, (ncr, nown, nb) = _sided_compose(pkg, entries, dx + u, x0, {0: sg, 2: si}, friction, moving)
            assert ncr >= 13 and nown >= 13 and nb >= 3, (which, friction, moving, ncr, nown, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "friction", "moving"])
@pytest.mark.parametrize("which", ["short", "full"])
def test_sided_kernel_equals_host_composition(pkg, which, case):
    """65 nodes, one local step of the collision batch alone with the sides installed by set_collision_sides: z and u bitwise equal to the
    host composition of shape_query, Mesh.query, Mesh.query_sided, mesh_velocity_query and the friction queries in list order"""
    friction, moving = case != "plain", case == "moving"
    entries = _sided_lists()[which]
    dx, x0, u, sg, si = _sided_case()
    s, b = _sided_system(pkg, entries, x0, friction, moving)
    assert s.collision_form() == 6
    s.set_collision_sides(0, sg); s.set_collision_sides(2, si)
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    want, counts = _sided_compose(pkg, entries, dx + u, x0, {0: sg, 2: si}, friction, moving)
    print("%s list, %s: crossed %d, pushed on their own side %d, boundary hits with a side %d" % ((which, case) + counts))
    assert counts[0] >= 13 and counts[1] >= 13 and counts[2] >= 3
    assert np.array_equal(r["z"], want), (np.abs(r["z"] - want).max(), np.flatnonzero((r["z"] != want).any(1)))
    assert np.array_equal(r["u"], u + (dx - want))
    unsided, _ = _sided_compose(pkg, entries, dx + u, x0, {}, friction, moving)      # what the shell kernel would give
    assert ((unsided != want).any(1)).sum() >= 13


@pytest.mark.gpu
def test_sided_kernel_with_a_self_colliding_sheet(pkg):
    """the folded strip of the self-collision kernel test (113 nodes that collide with their own sheet, 17 free particles) with side
    memory on the sheet: after a latch the sheet's own nodes hold side 0 and the free particles near it a side; one local step gives,
    bit for bit, query_excluding for the sheet's nodes (the self kernel's rule) and query_sided for the particles"""
    import test_sheet_self_collision as ts
    x0, F, skip, disp = ts._kernel_scene(pkg)
    entries = ts._kernel_lists(False)["short"]
    nv, n = len(x0) - ts.N_FREE, len(x0)
    reach = 0.25
    rng = np.random.default_rng(151)
    x0 = x0.copy()
    x0[nv:, 1] = np.where(np.arange(ts.N_FREE) % 2, ts.GAP_K + rng.uniform(0.1, 0.2, ts.N_FREE), -rng.uniform(0.1, 0.2, ts.N_FREE))      # above / below the strip
    x0[nv:, 0] = rng.uniform(-0.3, 0.3, ts.N_FREE); x0[nv:, 2] = rng.uniform(0.2, 1.2, ts.N_FREE)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x0.ravel(), np.ones(3 * n))
    b = s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
    mid = s.add_sheet_surface(0, nv, F, ts.R_K, self_collision=True)
    Vc, Fc = _cube()
    s.add_collision_mesh(0.3 * Vc, Fc)
    s.set_collision_mesh_side_memory(mid, reach)
    s.set_collision_shapes([e[0] for e in entries], [e[1] for e in entries])
    s.initialize()
    assert s.collision_form() == 6
    s.set_collision_sides(mid, rng.integers(-1, 2, n).astype(np.int32) * (np.arange(n) >= nv))
    s.latch_collision_sides()
    sheet = pkg.Mesh(x0[:nv], F, ts.R_K); sheet.F = F
    sheet.set_vertices(x0[:nv])
    side = s.collision_sides(mid)
    assert not side[:nv].any() and np.array_equal(side[nv:], sheet.side_latch(x0[nv:], side[nv:], reach)) and (side[nv:] != 0).sum() >= 8
    u = 0.001 * rng.normal(size=x0.shape)
    dx = x0 + disp
    dx[nv:, 1] = rng.uniform(0.02, ts.GAP_K - 0.02, ts.N_FREE)                         # the particles' candidates lie between the flaps: across one of them
    s.write_local(b, u=u)
    s.local_step_dx(b, dx)
    r = s.read_local(b)
    cube = pkg.Mesh(0.3 * Vc, Fc)
    p = dx + u
    ncr = 0
    for ty, par, f, mu in entries:
        if ty != MESH:
            q, _ = pkg.shape_query(ty, par, p, f)
        elif int(par[3]) == 0:
            q = sheet.query_excluding(p, skip, par[:3])[0]
            qs, _, _, cr = sheet.query_sided(p[nv:], side[nv:], reach, par[:3])
            q[nv:] = qs; ncr += int(cr.sum())
        else:
            proj, sd = cube.query(p, par[:3], frame=f)
            q = np.where((sd > 0)[:, None], proj, p)
        p = q
    own = (p[:nv] != (dx + u)[:nv]).any(1).sum()
    print("self-colliding strip with memory: %d of its own nodes moved, %d of %d particles crossed" % (own, ncr, ts.N_FREE))
    assert own >= nv / 5 and ncr >= 4
    assert np.array_equal(r["z"], p), np.flatnonzero((r["z"] != p).any(1))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 9: no memory set, nothing changes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_memory_no_change(pkg):
    """the drop scene of test_collision_shell (65 particles, a floor, a closed cube, an open sheet registered): with the sheet in the list
    the frames, collision_form and graph_state are those of a context built the same way; a context where the sheet has memory shows
    form 6 exactly while the list names the sheet, and with the sheet far away its frames are still the same bits"""
    x = _drop_scene()
    a, b = _drop_system(pkg, x, True), _drop_system(pkg, x, True)
    near = (a.base[0] + [MESH], a.base[1] + [[0.0, 0.25, 0, a.sheet]])
    a.set_collision_shapes(*near); b.set_collision_shapes(*near)
    assert a.collision_form() == b.collision_form() == 4
    ra, rb = _run(a, 4), _run(b, 4)
    assert _same_frames(ra, rb) and a.graph_state() == b.graph_state() and a.graph_state()["frame_graph_iters"] == 10
    _expect(pkg, lambda: a.collision_sides(a.sheet), "error 1", "no side memory")
    a.latch_collision_sides(); a.reset_collision_sides()                               # nothing to latch or reset: no effect
    assert _same_frames(_run(a, 2), _run(b, 2)) and a.graph_state() == b.graph_state()
    # the same scene with memory on the sheet, built by hand (the reach is set before initialize)
    Vc, Fc = _cube()
    c = pkg.System(device_id=0)
    c.set_timestep(DT)
    c.add_nodes(x.ravel(), np.ones(x.size))
    c.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    c.add_gravity([0.0, -G, 0.0])
    cube = c.add_collision_mesh(0.6 * Vc, Fc)
    sheet = c.add_collision_mesh(pkg.Mesh(*_grid(), 0.125), None)
    c.set_collision_mesh_side_memory(sheet, 0.5)
    c.set_collision_shapes(*a.base)
    c.initialize()
    d = _drop_system(pkg, x, True)
    assert c.collision_form() == 0 and _same_frames(_run(c, 3), _run(d, 3)) and c.graph_state() == d.graph_state()
    far = (a.base[0] + [MESH], a.base[1] + [[50.0, 0, 0, sheet]])
    c.set_collision_shapes(*far); d.set_collision_shapes(*far)
    assert c.collision_form() == 6 and d.collision_form() == 4
    g = c.graph_state()
    assert not g["iter_graph"] and g["frame_graph_iters"] == 0, g                      # dropped on the change of form
    assert _same_frames(_run(c, 3), _run(d, 3))
    assert c.graph_state()["frame_graph_iters"] == 10 and not c.collision_sides(sheet).any()
    c.set_collision_shapes(*a.base)
    assert c.collision_form() == 0 and c.graph_state()["frame_graph_iters"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 10: no tunnelling; GPU 13: launch modes and shards; GPU 14: checkpoint
# ---------------------------------------------------------------------------------------------------------------------------------
DT_T = 0.04
R_T = 0.01
SPEED_T = 3.0         # 12 r per frame
N_IN = 90


def _tunnel_scene():
    """130 particles 0.1 to 0.3 above a flat sheet (r = 0.01) falling at 3 m/s: 90 over its interior, 40 beside it"""
    rng = np.random.default_rng(161)
    n = 130
    x = np.zeros((n, 3))
    x[:N_IN, 0] = rng.uniform(-0.4, 0.4, N_IN); x[:N_IN, 2] = rng.uniform(-0.4, 0.4, N_IN)
    side = rng.uniform(size=n - N_IN) < 0.5
    far = rng.uniform(0.5 + 0.05, 0.9, n - N_IN) * np.where(rng.uniform(size=n - N_IN) < 0.5, -1, 1)
    near = rng.uniform(-0.9, 0.9, n - N_IN)
    x[N_IN:, 0] = np.where(side, far, near); x[N_IN:, 2] = np.where(side, near, far)
    # heights from which no frame's free-fall position comes within 3 r of the mid-surface: without memory no candidate then finds a
    # triangle within r, whatever the iteration (symplectic Euler: y_k = y_0 - k dt speed - g dt^2 k (k + 1) / 2)
    k = np.arange(1, 12)
    y = rng.uniform(0.1, 0.3, 4 * n)
    yk = y[:, None] - k[None] * DT_T * SPEED_T - G * DT_T * DT_T * (k * (k + 1) / 2)[None]
    y = y[(np.abs(yk) > 3 * R_T).all(1)]
    assert len(y) >= n
    x[:, 1] = y[:n]
    v = np.zeros((n, 3)); v[:, 1] = -SPEED_T
    return x, v


def _tunnel_system(pkg, x, v, kind, reach=2.0, rank=0, world=1, mass=1.0):
    """kind "memory": the sheet with side memory; "plain": the sheet without; "floor": a floor at y = r; "free": a far-away floor"""
    s = pkg.System(device_id=0)
    s.set_timestep(DT_T)
    s.add_nodes(x.ravel(), np.full(x.size, mass))
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    if world > 1:
        s.set_shard(rank, world); s.set_shard_mode("subtree")
    s.sheet = s.add_collision_mesh(pkg.Mesh(*_grid(), R_T), None)
    if kind == "memory":
        s.set_collision_mesh_side_memory(s.sheet, reach)
    if kind in ("memory", "plain"):
        s.set_collision_shapes([MESH], [[0, 0, 0, s.sheet]])
    else:
        s.set_collision_shapes([FLOOR], [[0, R_T if kind == "floor" else -100.0, 0, 0]])
    s.kind, s.v0 = kind, v
    return s


def _tunnel_frames(s, frames=20, iters=20, start=True):
    if start:
        s.m_v = s.v0.ravel()
    xs, vs, sd = [], [], []
    for _ in range(frames):
        s.step(iters)
        xs.append(s.m_x.reshape(-1, 3).copy()); vs.append(s.m_v.reshape(-1, 3).copy())
        sd.append(s.collision_sides(s.sheet) if s.kind == "memory" else np.zeros(len(xs[-1]), np.int32))
    return np.array(xs), np.array(vs), np.array(sd)


@pytest.mark.gpu
def test_fast_particles_do_not_tunnel(pkg):
    """130 particles fall at 3 m/s (12 r a frame at dt = 0.04, r = 0.01) onto a flat sheet with reach 2; 20 frames x 20 iterations.  The
    first candidates land far beyond r below the mid-surface.  With memory the 90 over the sheet follow, to 1e-9, the same particles
    over a floor at y = r (the reference and tolerance of test_free_particles_on_a_flat_sheet); without memory every one of them ends
    below y = -r: its candidate finds no triangle within r.  The 40 beside the sheet stay bitwise in free fall in both runs.  Measured on
    the MI355X: with memory |x - floor| 6.42e-14, |v - floor| 1.62e-13; the control ends at y in [-5.592, -5.436]."""
    x, v = _tunnel_scene()
    runs = {}
    for kind in ("memory", "plain", "floor", "free"):
        s = _tunnel_system(pkg, x, v, kind); s.initialize()
        assert s.collision_form() == {"memory": 6, "plain": 4}.get(kind, 0)
        runs[kind] = _tunnel_frames(s)
    xm, vm, sd = runs["memory"]; xp, vp, _ = runs["plain"]; xf, vf, _ = runs["floor"]; xc, vc, _ = runs["free"]
    below = (x[:N_IN, 1] + 3 * DT_T * v[:N_IN, 1] < -R_T).sum()                        # three frames at the start speed alone end beyond r below
    ex, ev = np.abs(xm[:, :N_IN] - xf[:, :N_IN]).max(), np.abs(vm[:, :N_IN] - vf[:, :N_IN]).max()
    print("fast particles: with memory |x - floor| %.3g, |v - floor| %.3g; control ends at y in [%.3f, %.3f]; %d candidates beyond r below within three frames"
          % (ex, ev, xp[-1, :N_IN, 1].min(), xp[-1, :N_IN, 1].max(), below))
    assert below == N_IN
    assert ex <= 1e-9 and ev <= 1e-9, (ex, ev)
    assert (sd[:, :N_IN] == 1).all() and np.abs(xm[-1, :N_IN, 1] - R_T).max() < 1e-3
    assert (xp[-1, :N_IN, 1] < -R_T).all()
    for xs, vs in ((xm, vm), (xp, vp)):
        assert np.array_equal(xs[:, N_IN:], xc[:, N_IN:]) and np.array_equal(vs[:, N_IN:], vc[:, N_IN:])


def _tunnel_mode_results(pkg):
    x, v = _tunnel_scene()
    s = _tunnel_system(pkg, x, v, "memory"); s.initialize()
    xs, vs, sd = _tunnel_frames(s, 8)
    return dict(x=xs, v=vs, side=sd)


def _child_main(path):
    from __graft_entry__ import load_package
    np.savez(path, **_tunnel_mode_results(load_package()))


@pytest.mark.gpu
def test_side_memory_launch_modes_bitwise(pkg, monkeypatch, tmp_path):
    """graph, eager, ADMM_HIP_FRAME_GRAPH=0 in this process and ADMM_HIP_LOCAL_MULTI=0 in a fresh child process: eight frames of the
    fast particles and their sides, bit for bit"""
    res = {}
    for env in ({}, {"ADMM_HIP_GRAPH": "0"}, {"ADMM_HIP_FRAME_GRAPH": "0"}):
        for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH", "ADMM_HIP_LOCAL_MULTI"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res[tuple(env.items())] = _tunnel_mode_results(pkg)
    keys = list(res)
    for k in keys[1:]:
        for name, v in res[keys[0]].items():
            assert np.array_equal(res[k][name], v), (k, name)
    for k in ("ADMM_HIP_GRAPH", "ADMM_HIP_FRAME_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, ADMM_HIP_LOCAL_MULTI="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_side_memory as t; t._child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.load(path)
    for name, v in res[keys[0]].items():
        assert np.array_equal(got[name], v), name
    assert (res[keys[0]]["side"][-1, :N_IN] == 1).all()


@pytest.mark.gpu
def test_side_memory_two_subtree_shards(pkg, monkeypatch):
    """the fast particles in two subtree shards: the ranks' frames and sides bitwise equal, and within 1e-9 of one rank"""
    import threading
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    x, v = _tunnel_scene()
    ref = _tunnel_system(pkg, x, v, "memory"); ref.initialize()
    rx, rv, rs = _tunnel_frames(ref, 8)
    shards = [_tunnel_system(pkg, x, v, "memory", rank=r, world=2) for r in range(2)]
    hooks = _thread_allreduce_hooks(2)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    for s in shards:
        s.m_v = v.ravel()
    res, errs = [None, None], []

    def run(r):
        try:
            res[r] = _tunnel_frames(shards[r], 8, start=False)
        except Exception as e:  # noqa: BLE001
            errs.append((r, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join(timeout=300)
    assert not errs, errs
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert np.abs(res[0][0] - rx).max() < 1e-9 and np.array_equal(res[0][2], rs)


@pytest.mark.gpu
def test_checkpoint_with_sides(pkg):
    """5 frames of the fast particles, then x, v, u and the sides are read; a fresh context resumed from them gives bitwise the next 5
    frames; the same resume without the sides differs.  The particles are heavy here (mass 10 against dt^2 w^2 = 1.64) and a frame has 2
    iterations, so a particle that crossed within the frame ends it still below the mid-surface, where only the remembered side tells
    above from below (asserted: some node with side +1 is below the mid-surface at the save); staggered heights make some arrive in
    every frame.  Measured on the MI355X: 32 nodes across at the save, 35 nodes differ in the resume without the sides."""
    x, v = _tunnel_scene()
    x[:, 1] = np.linspace(0.05, 0.65, len(x))
    a = _tunnel_system(pkg, x, v, "memory", mass=10.0); a.initialize()
    _tunnel_frames(a, 5, iters=2)
    X, V, S = a.m_x.copy(), a.m_v.copy(), a.collision_sides(a.sheet)
    U = a.read_local(0)["u"].copy()
    xa = _tunnel_frames(a, 5, iters=2, start=False)
    across = (X.reshape(-1, 3)[:N_IN, 1] < 0) & (S[:N_IN] == 1)
    print("checkpoint: %d nodes below the mid-surface with side +1 at the save" % across.sum())
    assert across.any()
    out = {}
    for with_sides in (True, False):
        b = _tunnel_system(pkg, x, v, "memory", mass=10.0); b.initialize()
        b.m_x = X; b.m_v = V
        b.write_local(0, u=U)
        if with_sides:
            b.set_collision_sides(b.sheet, S)
        out[with_sides] = _tunnel_frames(b, 5, iters=2, start=False)
    for p, q in zip(xa, out[True]):
        assert np.array_equal(p, q)
    differ = (out[False][0] != xa[0]).any(2).any(0)
    print("checkpoint: resumed without the sides, %d nodes differ" % differ.sum())
    assert differ.sum() >= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU 11: a swept sheet; GPU 12: a tet block dropped fast onto a sheet
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_swept_sheet_keeps_particles_on_their_side(pkg):
    """resting particles (no gravity) on either side of a vertical sheet (r = 0.01) that the caller moves by 5 r per frame through
    set_collision_shapes, 12 frames.  With memory every particle in the sheet's path stays on the side it was latched on and ends at
    least r from the mid-surface; without memory the sheet passes particles by: at least one is left behind on the far side.  Measured
    on the MI355X: smallest distance with memory 0.0100, 104 of 104 left behind in the control."""
    r, step, frames = 0.01, 0.05, 12
    rng = np.random.default_rng(171)
    n = 130
    x = np.stack([rng.uniform(0.05, 0.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)], 1)      # ahead of the sheet, which starts at x = 0
    x[::5, 0] = -rng.uniform(0.05, 0.3, len(x[::5]))                                 # ... and some behind it
    f = _frame(_quarter(2, 1), [0.0, 0.0, 0.0])                                      # the grid's normal +y turned to -x: the sheet lies in the plane x = t
    res = {}
    for memory in (True, False):
        s = pkg.System(device_id=0)
        s.set_timestep(DT_T)
        s.add_nodes(x.ravel(), np.ones(x.size))
        s.add_forces(KIND["COLLISION"], np.arange(n, dtype=np.int32), [W])
        sheet = s.add_collision_mesh(pkg.Mesh(*_grid(), r), None)
        if memory:
            s.set_collision_mesh_side_memory(sheet, 1.0)
        s.set_collision_shapes([MESH], [[0, 0, 0, sheet]])
        s.initialize()
        s.set_collision_frames([f])
        for k in range(frames):
            # the frame turns about the origin, the translation is applied in local coordinates: local y = -x world, so t_y = -position
            s.set_collision_shapes([MESH], [[0, -k * step, 0, sheet]])
            s.step(20)
        res[memory] = (s.m_x.reshape(-1, 3).copy(), s.collision_sides(sheet) if memory else None)
    pos = (frames - 1) * step
    (xm, sd), (xp, _) = res[True], res[False]
    ahead = x[:, 0] > 0
    print("swept sheet at x = %.2f: with memory min distance of the particles in its path %.4f; control: %d of %d left behind"
          % (pos, (xm[ahead, 0] - pos).min(), int((xp[ahead, 0] < pos).sum()), int(ahead.sum())))
    assert (sd[ahead] == -1).all() and (sd[~ahead] == 1).all()                        # ahead: the side the normals point away from
    assert (xm[ahead, 0] - pos >= r - 1e-9).all()
    assert np.abs(xm[~ahead] - x[~ahead]).max() < 1e-12                               # behind it: never touched
    assert (xp[ahead, 0] < pos).sum() >= 1


def _fast_block(pkg, memory, speed, frames=10, iters=20):
    """the block of test_block_lands_on_a_sheet (a 2 x 2 x 2-cell tet block 0.3 wide over a fully anchored 5 x 5-node cloth at y = 0,
    r = 0.125), released with a downward speed"""
    from test_collision_shell import NC, R_CLOTH
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
    if memory:
        s.set_collision_mesh_side_memory(mid, 1.0)
    s.set_collision_shapes([MESH], [[0, 0, 0, mid]])
    s.initialize()
    v = np.zeros_like(x); v[NC:, 1] = -speed
    s.m_v = v.ravel()
    ys = []
    for _ in range(frames):
        s.step(iters)
        ys.append(s.m_x.reshape(-1, 3)[NC:, 1].min())
    return np.array(ys), s.body_surface_status(mid), s.m_x.reshape(-1, 3)[:NC, 1].copy()


@pytest.mark.gpu
def test_fast_block_lands_on_a_sheet(pkg):
    """the tet block of test_block_lands_on_a_sheet released at 4 r / dt = 25 m/s downwards.  With memory no node is below the sheet's
    plane after 10 frames and no frame's surface update is refused.  The control without memory is printed only.  Measured on the MI355X:
    lowest node after ten frames 0.4229 with memory (-0.2826, -0.4513, -0.1759 after the first three: it is brought back), -5.1351 in
    the control."""
    from test_collision_shell import R_CLOTH
    speed = 4 * R_CLOTH / DT
    ys, st, cloth = _fast_block(pkg, True, speed)
    yc, _, _ = _fast_block(pkg, False, speed)
    print("fast block (%.1f m/s): lowest node per frame with memory %s; after ten frames %.4f (memory), %.4f (control)" % (speed, np.round(ys, 4).tolist(), ys[-1], yc[-1]))
    assert st["refused"] == 0 and st["updated"] == 10
    assert np.abs(cloth).max() < 1e-3
    assert ys[-1] > cloth.max()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU 6 / GPU 15: the class API
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_side_memory_program_compiles(pkg):
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_side_memory", pkg))


R_CS, REACH_CS, MESH_TY, VY_CS = 0.03125, 1.0, -0.375, -4.0


def _class_scene_system(pkg):
    """the cloth scene of test_collision_shell (a 5 x 5-node cloth, corners anchored, 65 particles above it) with side memory on the
    cloth's sheet surface and on an open obstacle mesh below it (the cloth's rest triangles), thin shells and fast particles"""
    from test_collision_shell import NC, _cloth_scene
    x, m, F, corners = _cloth_scene()
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TRI_STRAIN"], F, [100.0, 0.95, 1.05, 1.0])
    s.add_forces(KIND["BEND"], pkg.meshgen.bend_hinges(F), [20.0])
    s.add_forces(KIND["ANCHOR"], corners, [-1.0, 1.0])
    s.add_forces(KIND["COLLISION"], np.arange(len(x), dtype=np.int32), [W])
    s.add_gravity([0.0, -G, 0.0])
    s.sheet = s.add_sheet_surface(0, NC, F, R_CS)
    s.set_collision_mesh_side_memory(s.sheet, REACH_CS)
    s.obst = s.add_collision_mesh(pkg.Mesh(x[:NC], F, R_CS), None)
    s.set_collision_mesh_side_memory(s.obst, REACH_CS)
    s.set_collision_shapes([MESH, MESH], [[0, 0, 0, s.sheet], [0, MESH_TY, 0, s.obst]])
    s.initialize()
    v = np.zeros_like(x); v[NC:, 1] = VY_CS
    s.m_v = v.ravel()
    return s, x, m, F, corners


@pytest.mark.gpu
def test_class_api_side_memory(pkg, tmp_path):
    """scene_side_memory.cpp -- admm::System with CollisionSheet::side_reach and CollisionMesh::side_reach in one CollisionForce's list --
    gives bitwise the C ABI's frames; the particles over the cloth end above it"""
    from test_collision_shell import NC
    from test_cpp_host import compile_cpp
    exe = compile_cpp("scene_side_memory", pkg)
    s, x, m, F, corners = _class_scene_system(pkg)
    assert s.collision_form() == 6
    hinges = pkg.meshgen.bend_hinges(F)
    frames, iters = 6, 10
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([len(x), len(F), len(hinges), len(corners), NC], np.int32).tofile(f)
        x.astype(np.float64).tofile(f); m.astype(np.float64).tofile(f)
        for a in (F, hinges, corners):
            np.asarray(a).astype(np.int32).tofile(f)
        np.array([R_CS, DT, REACH_CS, R_CS, REACH_CS, MESH_TY, VY_CS]).tofile(f)
    r = subprocess.run([exe, inp, outp, str(frames), str(iters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = np.fromfile(outp).reshape(frames, 2, len(x) * 3)
    for k in range(frames):
        s.step(iters)
        assert np.array_equal(got[k, 0], s.m_x) and np.array_equal(got[k, 1], s.m_v), (k, np.abs(got[k, 0] - s.m_x).max())
    side = s.collision_sides(s.sheet)
    assert not side[:NC].any() and (side[NC:] == 1).sum() >= 20
