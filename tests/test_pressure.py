"""Pressure chambers (include/admm_hip.h "pressure chambers"; csrc/pressure.hpp, kernels_pressure.hpp, abi_pressure.inc,
pressure_host.cpp).

CPU: pressure_query against a numpy.longdouble restatement of the rule to a bound derived from the operation order and the summation
tree, the exact identities of the load on closed chambers, and the refusals a host-only context can show.
GPU: the device's v and records against the host twin bit for bit (chambers of 1 .. 16 449 triangles at triangle offsets that are no
multiples of 64, through a permuted node order), off is off, the launch modes, the solver's options, two shards, an inflating bar, the
C++ class mirror.

The rounding bound, first order in EPS (u), every input an exact double.
  A triangle.  a = x1 - x0, b = x2 - x0 carry one rounding each, a component of n = a x b two products and a difference on top of
them: |dn_j| <= gamma(4) (|a| x |b|)_j, the cross product with every minus a plus.  vol = (r0 . (r1 x r2)) / 6: one rounding in every
r_k, four in the cross product's components, a product, two sums and the division: |dvol| <= gamma(9) (|r0| . (|r1| x |r2|)) / 6.
area = 0.5 sqrt(n . n): |d(n . n)| <= 2 sum |n_j| |dn_j| + gamma(3) n . n, through the root d / (2 |n|) + u |n|, the half is exact.
  A sum runs through a fixed tree: the wave butterfly (6 additions on the way to lane 0), the reducer's strided loop
(ceil(nb / 256) additions, nb = ceil(nt / 64)) and its LDS fold (8): depth D = 6 + ceil(nb / 256) + 8 roundings on any path, so
|computed - exact| <= gamma(D + k) sum |term| with k the term's own roundings and |term| its cancellation-free magnitude above (V: k =
9, N: k = 4), and for A the terms' errors plus gamma(D) sum area.
  The law.  Constant: p is the caller's double.  Gas: q = amount / V inherits |q| dV / (V - dV) and the division's u |q|, p = q - ambient
one more rounding.  resultant = p N: dp |N| + |p| dN + u |p N|.
  A node.  A corner adds p g, g = n_j / 6: |d(p g)| <= dp |g| + |p| (dn_j / 6 + u |g|) + u |p g|; the sequential sum of k corners adds
gamma(k) sum |p g|; dv = (dt f) / m: dt df / m + gamma(2) |dv|."""
import threading

import numpy as np
import pytest

from checkers import EPS, KIND, gamma

L = np.longdouble
LEPS = L(np.finfo(np.longdouble).eps)
DT = 0.04
G = np.array([0.0, -9.8, 0.0])
FLOOR = 0
ERR_ARG, ERR_HIP, ERR_STATE = 1, 2, 3
SIZES = [1, 2, 63, 64, 65, 129, 257 * 64 + 1]      # the last: 257 full blocks and one triangle, the reducer's strided loop wraps
FIELDS = ("volume", "area", "area_vector", "pressure", "resultant", "n_tris", "collapsed")


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule in long double, with its error bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _depth(nt):
    nb = (nt + 63) // 64
    return 6 + (nb + 255) // 256 + 8


def _abscross(a, b):
    """|a| x |b| with every minus a plus: the magnitude a rounded cross product's error is measured against"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _active(c):
    if c.get("mode", "constant") == "gas":
        return c.get("amount", 0.0) != 0.0 or c.get("ambient", 0.0) != 0.0
    return c.get("p", 0.0) != 0.0


def _reference(x, m, chambers, dt):
    """-> (records, record bounds, dv, dv bound): the rule of csrc/pressure.hpp in long double and the first-order rounding bound of the
    double evaluation (module docstring)"""
    x, m, u = L(x).reshape(-1, 3), L(m), L(EPS)
    nv = len(x)
    f, e_f, mag = np.zeros((nv, 3), L), np.zeros((nv, 3), L), np.zeros((nv, 3), L)
    cnt = np.zeros(nv, np.int64)
    vals, bnds = [], []
    for c in chambers:
        t = np.asarray(c["tris"], dtype=np.int64).reshape(-1, 3)
        D = _depth(len(t))
        o = x[t[0, 0]]
        x0, x1, x2 = x[t[:, 0]], x[t[:, 1]], x[t[:, 2]]
        a, b = x1 - x0, x2 - x0
        n, an = np.cross(a, b), _abscross(a, b)
        e_n = gamma(4) * an
        r0, r1, r2 = x0 - o, x1 - o, x2 - o
        vol = (r0 * np.cross(r1, r2)).sum(1) / 6
        volabs = (np.abs(r0) * _abscross(r1, r2)).sum(1) / 6
        nn = (n * n).sum(1)
        ln = np.sqrt(nn)
        assert (ln > 0).all()
        e_area = L(0.5) * ((2 * (np.abs(n) * e_n).sum(1) + gamma(3) * nn) / (2 * ln) + u * ln)
        V, A, N = vol.sum(), (ln / 2).sum(), (n / 2).sum(0)
        e_V = gamma(D + 9) * volabs.sum()
        e_A = e_area.sum() * (1 + gamma(D)) + gamma(D) * (ln / 2).sum()
        e_N = gamma(D + 4) * (an / 2).sum(0)
        if c.get("mode", "constant") == "gas":
            amount, ambient = L(c.get("amount", 0.0)), L(c.get("ambient", 0.0))
            collapsed = int(not V - e_V > 0)
            if collapsed:      # (V <= 0 beyond doubt, or exactly 0 as for a single triangle, whose only term is about its own corner)
                assert V + e_V < 0 or (V == 0 and e_V == 0), "the reference cannot tell on which side of 0 the double volume falls"
                p, e_p = L(0.0), L(0.0)
            else:
                assert e_V < 1e-6 * V, "the reference assumes a gas chamber far from collapse"
                q = amount / V
                e_q = np.abs(q) * e_V / (V - e_V)
                e_q = e_q + u * (np.abs(q) + e_q)
                p = q - ambient
                e_p = e_q + u * (np.abs(p) + e_q)
        else:
            p, e_p, collapsed = L(c.get("p", 0.0)), L(0.0), 0
        res = p * N
        e_res = e_p * np.abs(N) + (np.abs(p) + e_p) * e_N + u * np.abs(res)
        vals.append(dict(volume=V, area=A, area_vector=N, pressure=p, resultant=res, n_tris=len(t), collapsed=collapsed))
        bnds.append(dict(volume=e_V, area=e_A, area_vector=e_N, pressure=e_p, resultant=e_res))
        if not _active(c):
            continue
        g = n / 6
        term = p * g
        e_term = e_p * np.abs(g) + (np.abs(p) + e_p) * (e_n / 6 + u * np.abs(g)) + u * np.abs(term)
        for j in range(3):
            np.add.at(f, t[:, j], term); np.add.at(e_f, t[:, j], e_term); np.add.at(mag, t[:, j], np.abs(term)); np.add.at(cnt, t[:, j], 1)
    k = L(cnt)[:, None]
    e_f = e_f + (k * u / (1 - k * u)) * mag
    dv = L(dt) * f / m[:, None]
    e_dv = L(dt) * e_f / m[:, None] + gamma(2) * np.abs(dv)
    return vals, bnds, dv, e_dv


def _soup(rng, nodes, nt, anchor=None):
    """nt random triangles over `nodes`, three distinct nodes each (the first triangle starts at `anchor` if given); three in four of them
    turned so that their volume term about the chamber's origin is not negative -- V stays well above zero, with cancellation left in"""
    nodes = np.asarray(nodes)
    t = np.stack([rng.permutation(len(nodes))[:3] for _ in range(nt)]) if len(nodes) < 64 else None
    if t is None:
        t = rng.integers(0, len(nodes), (nt, 3))
        bad = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
        while bad.any():
            t[bad] = rng.integers(0, len(nodes), (int(bad.sum()), 3))
            bad = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    t = nodes[t]
    if anchor is not None:
        if anchor in t[0]:
            t[0] = np.roll(t[0], -int(np.flatnonzero(t[0] == anchor)[0]))
        else:
            t[0, 0] = anchor
    return t.astype(np.int32)


def _orient(x, t, rng):
    o = x[t[0, 0]]
    vol = np.einsum("ij,ij->i", x[t[:, 0]] - o, np.cross(x[t[:, 1]] - o, x[t[:, 2]] - o))
    flip = (vol < 0) & (rng.random(len(t)) < 0.75)
    flip[0] = False
    t = t.copy()
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def _fan(rng, hub, others, nt):
    """nt triangles that all name `hub`, in any corner"""
    t = np.empty((nt, 3), np.int32)
    others = np.setdiff1d(others, [hub])
    for k in range(nt):
        a, b = rng.choice(others, 2, replace=False)
        t[k] = np.roll([hub, a, b], k % 3)
    return t


def _particles(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, 3)) + [0.5, -0.3, 0.2], rng.uniform(0.5, 2.0, n)


def _check(got_recs, got_dv, vals, bnds, dv, e_dv, tag):
    worst = 0.0
    tiny = L(2.0) ** -1074
    for c, (r, val, bnd) in enumerate(zip(got_recs, vals, bnds)):
        assert r["n_tris"] == val["n_tris"] and r["collapsed"] == val["collapsed"]
        for k in ("volume", "area", "area_vector", "pressure", "resultant"):
            err, b = np.abs(L(r[k]) - val[k]), bnd[k] + tiny
            assert np.all(err <= b), (tag, c, k, err, b)
            if np.all(bnd[k] > 0):
                worst = max(worst, float(np.max(err / b)))
    err, b = np.abs(L(got_dv) - dv), e_dv + tiny
    assert (err <= b).all(), (tag, "dv", float((err / b).max()))
    return max(worst, float((err / b).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", SIZES)
def test_pressure_query_against_long_double(pkg, nt):
    """an open soup of nt triangles over random particles, in both modes, next to a second chamber: 70 triangles that all name particle
    0 (a hub in more than 64 triangles), which the soup's first triangle names too, so that particle is in two chambers.  V, A, N, p,
    the resultant and dv within the bound of the module docstring (nt = 16 449: D = 16); the bound is first order in EPS and is not
    fitted to the result (the largest ratio seen is printed)"""
    rng = np.random.default_rng(500 + nt)
    nv = 12 if nt < 63 else 400
    x, m = _particles(nv, 300 + nt)
    soup = _orient(x, _soup(rng, np.arange(nv), nt, anchor=0), rng)
    hub = _fan(rng, 0, np.arange(1, nv), 70)
    assert (hub == 0).sum() == 70 and (soup == 0).any()
    worst = 0.0
    for law in (dict(mode="constant", p=-3.5), dict(mode="gas", amount=0.7, ambient=1.25)):
        chambers = [dict(tris=soup, **law), dict(tris=hub, mode="constant", p=2.25)]
        dv, recs = pkg.pressure_query(x, m, chambers, DT)
        vals, bnds, rdv, e_dv = _reference(x, m, chambers, DT)
        worst = max(worst, _check(recs, dv, vals, bnds, rdv, e_dv, (nt, law["mode"])))
        assert np.isfinite(dv).all() and dv[0].any()
        untouched = np.setdiff1d(np.arange(nv), np.concatenate([soup.ravel(), hub.ravel()]))
        assert not dv[untouched].any()
    print("pressure_query, %d triangles: depth %d, max error / bound = %.3f" % (nt, _depth(nt), worst))


def _closed(pkg, name):
    mg = pkg.meshgen
    if name == "tet":
        x = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.2, 1.1, 0.4], [0.3, 0.2, 1.5]])
        return x, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    xb, tets = mg.bar(2, 2, 3 if name == "bar3" else 4)
    rng = np.random.default_rng(11)
    return xb + 0.004 * rng.normal(size=xb.shape), mg.tet_surface(tets)


@pytest.mark.parametrize("name", ["tet", "bar3", "bar4"])
def test_exact_identities_on_closed_chambers(pkg, name):
    """closed chambers (a tetrahedron, the surfaces of meshgen.bar(2, 2, 3) -- 64 triangles -- and bar(2, 2, 4), nodes perturbed):
    f_i / p = m dv / (dt p) equals grad_i V = (1 / 6) sum over the node's fan of x_j x x_k, evaluated in long double, within the bound
    of dv (module docstring) scaled by m / (dt |p|); |sum f| and |sum x x f| lie within the sums of the nodes' bounds (both are zero in
    exact arithmetic), and so does the record's resultant within its own bound; a gas chamber with amount = ambient V (V the twin's
    double) gives |p| <= gamma(3) |ambient|: one rounding in the product ambient V, one in the division, the subtraction of two numbers
    that close is exact.  The long double evaluations themselves add a few of their own roundings, allowed for with the same
    magnitudes."""
    x, tris = _closed(pkg, name)
    nv = len(x)
    if name == "bar3":
        assert len(tris) == 64
    rng = np.random.default_rng(5)
    m = rng.uniform(0.5, 2.0, nv)
    p = 7.5
    ch = [dict(tris=tris, mode="constant", p=p)]
    dv, recs = pkg.pressure_query(x, m, ch, DT)
    vals, bnds, rdv, e_dv = _reference(x, m, ch, DT)
    _check(recs, dv, vals, bnds, rdv, e_dv, name)
    assert recs[0]["volume"] > 0
    xl = L(x)
    grad, gmag, fan = np.zeros((nv, 3), L), np.zeros((nv, 3), L), np.zeros(nv)
    for j in range(3):
        xa, xb = xl[tris[:, (j + 1) % 3]], xl[tris[:, (j + 2) % 3]]
        np.add.at(grad, tris[:, j], np.cross(xa, xb) / 6); np.add.at(gmag, tris[:, j], _abscross(xa, xb) / 6); np.add.at(fan, tris[:, j], 1)
    scale = L(m)[:, None] / (L(DT) * L(p))
    f_over_p = L(dv) * scale
    e_f = e_dv * scale
    slack = (8 + 4 * L(fan))[:, None] * LEPS * (gmag + np.abs(f_over_p))
    assert (np.abs(f_over_p - grad) <= e_f + slack).all(), float((np.abs(f_over_p - grad) / (e_f + slack)).max())
    assert (e_f + slack <= 1e-12 * np.abs(grad).max()).all()                      # the check binds
    f = f_over_p * L(p)
    e_force = e_f * L(p)
    lsl = 4 * nv * LEPS
    assert (np.abs(f.sum(0)) <= e_force.sum(0) + lsl * np.abs(f).sum(0)).all()
    tq, tq_b = np.cross(xl, f).sum(0), _abscross(xl, e_force).sum(0) + lsl * _abscross(xl, f).sum(0)
    assert (np.abs(tq) <= tq_b).all(), (tq, tq_b)
    assert (np.abs(L(recs[0]["resultant"])) <= bnds[0]["resultant"]).all()
    # gas at equilibrium
    V = recs[0]["volume"]
    for ambient in (1.0, 101325.0):
        _, r = pkg.pressure_query(x, m, [dict(tris=tris, mode="gas", amount=ambient * V, ambient=ambient)], DT)
        assert abs(r[0]["pressure"]) <= gamma(3) * ambient and r[0]["collapsed"] == 0, (ambient, r[0]["pressure"])


def test_translation_zero_pressure_and_orientation(pkg):
    """translating every node leaves dv within the bound: with coordinates on a 2^-20 grid and a translation by whole numbers x + T is
    exact, so a, b and r_k = x_k - o are the same doubles and dv is not just within the sum of the two bounds but the same bits (both
    asserted) -- with sums about the world's origin in place of o the volume would lose log2 |T| bits; p = 0 (and a gas chamber with
    amount = ambient = 0) leaves v bit for bit and reports the chamber's geometry all the same; a triangle listed with reversed
    orientation negates its terms exactly: V, N, the resultant and dv change sign bit for bit, A stays"""
    rng = np.random.default_rng(77)
    nv = 60
    x = np.round(rng.uniform(0.0, 1.0, (nv, 3)) * 2.0 ** 20) / 2.0 ** 20
    m = rng.uniform(0.5, 2.0, nv)
    soup = _orient(x, _soup(rng, np.arange(nv - 5), 65), rng)
    T = np.array([4096.0, -65536.0, 1024.0])
    for law in (dict(mode="constant", p=2.5), dict(mode="gas", amount=0.4, ambient=0.3)):
        ch = [dict(tris=soup, **law)]
        dv, r = pkg.pressure_query(x, m, ch, DT)
        dv2, r2 = pkg.pressure_query(x + T, m, ch, DT)
        assert np.array_equal((x + T) - T, x)
        _, _, _, e1 = _reference(x, m, ch, DT)
        _, _, _, e2 = _reference(x + T, m, ch, DT)
        assert (np.abs(L(dv2) - L(dv)) <= e1 + e2).all() and dv.any()
        assert np.array_equal(dv2, dv) and all(np.array_equal(r[0][k], r2[0][k]) for k in FIELDS)
    v0 = rng.normal(size=(nv, 3))
    for law in (dict(mode="constant", p=0.0), dict(mode="gas", amount=0.0, ambient=0.0)):
        dv, r = pkg.pressure_query(x, m, [dict(tris=soup, **law)], DT)
        assert (v0 + dv).tobytes() == v0.tobytes() and not dv.any() and not np.signbit(dv).any()
        assert r[0]["area"] > 0 and r[0]["pressure"] == 0.0 and r[0]["n_tris"] == 65 and r[0]["collapsed"] == (law["mode"] == "gas" and not r[0]["volume"] > 0)
    for tris in (soup[:1], soup):
        ch = [dict(tris=tris, mode="constant", p=-1.75)]
        dv, r = pkg.pressure_query(x, m, ch, DT)
        dvr, rr = pkg.pressure_query(x, m, [dict(tris=tris[:, [0, 2, 1]], mode="constant", p=-1.75)], DT)
        assert np.array_equal(dvr, -dv) and dv.any()
        assert rr[0]["volume"] == -r[0]["volume"] and rr[0]["area"] == r[0]["area"]
        assert np.array_equal(rr[0]["area_vector"], -r[0]["area_vector"]) and np.array_equal(rr[0]["resultant"], -r[0]["resultant"])
    # a gas chamber that is inside out collapses: p = 0, counted, nothing moves
    xt, tt = _closed(pkg, "tet")
    dv, r = pkg.pressure_query(xt, np.ones(4), [dict(tris=tt[:, [0, 2, 1]], mode="gas", amount=1.0, ambient=1.0)], DT)
    assert r[0]["collapsed"] == 1 and r[0]["pressure"] == 0.0 and r[0]["volume"] < 0 and not dv.any()


def _raises(pkg, code, words, fn, *a, **k):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*a, **k)
    msg = str(e.value)
    assert int(msg.split("error ")[1].split(":")[0]) == code, msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def _named_edge(msg):
    a, b = msg.split("edge (")[1].split(")")[0].split(",")
    return {int(a), int(b)}


def test_refusals_on_a_host_only_context(pkg):
    """every refusal names the offending value: nt < 1, a node id out of range, a triangle naming a node twice, an unknown mode, a
    non-finite parameter; in gas mode an open chamber at add (the edge named is one of the missing triangle's), a closed chamber with
    inward normals at initialize (chamber and volume named), and through set_pressure; add after initialize is a state error;
    chamber_state without a device is a state error"""
    mg = pkg.meshgen
    s = pkg.make_bar_system(2, 2, 3, device_id=-1)
    n = s.n_nodes
    _, tets = mg.bar(2, 2, 3)
    surf = mg.tet_surface(tets)
    assert s.add_pressure_chamber(surf[:5], "constant", p=2.0) == 0
    _raises(pkg, ERR_ARG, ["chamber 1", "nt 0"], s.add_pressure_chamber, np.zeros((0, 3), np.int32))
    _raises(pkg, ERR_ARG, ["triangle 1", "node %d" % n, "%d nodes" % n], s.add_pressure_chamber, [[0, 1, 2], [3, n, 4]])
    _raises(pkg, ERR_ARG, ["triangle 0", "node -1"], s.add_pressure_chamber, [[0, -1, 2]])
    _raises(pkg, ERR_ARG, ["triangle 2", "(7, 8, 7)", "twice"], s.add_pressure_chamber, [[0, 1, 2], [3, 5, 4], [7, 8, 7]])
    _raises(pkg, ERR_ARG, ["mode 7"], s.add_pressure_chamber, surf, 7)
    _raises(pkg, ERR_ARG, ["p nan"], s.add_pressure_chamber, surf, "constant", p=float("nan"))
    _raises(pkg, ERR_ARG, ["amount inf"], s.add_pressure_chamber, surf, "gas", amount=float("inf"), ambient=1.0)
    _raises(pkg, ERR_ARG, ["ambient -inf"], s.add_pressure_chamber, surf, "gas", amount=1.0, ambient=float("-inf"))
    hole = 17
    msg = _raises(pkg, ERR_ARG, ["chamber 1", "closed", "edge ("], s.add_pressure_chamber, np.delete(surf, hole, 0), "gas", amount=1.0, ambient=1.0)
    assert _named_edge(msg) <= set(int(v) for v in surf[hole])
    flipped = surf.copy(); flipped[9] = flipped[9][[0, 2, 1]]                # closed as a set, but one triangle runs the other way
    msg = _raises(pkg, ERR_ARG, ["closed", "edge ("], s.add_pressure_chamber, flipped, "gas", amount=1.0, ambient=1.0)
    assert _named_edge(msg) <= set(int(v) for v in surf[9])
    assert s.add_pressure_chamber(surf, "gas", amount=1.0, ambient=1.0) == 1    # nothing refused above was kept
    assert s.add_pressure_chamber(np.delete(surf, hole, 0), "constant", p=0.0) == 2
    s.set_pressure(0, "constant", p=-4.0)                                    # before finalize
    _raises(pkg, ERR_ARG, ["chamber 2", "closed", "edge ("], s.set_pressure, 2, "gas", amount=1.0, ambient=1.0)
    s.initialize()
    _raises(pkg, ERR_STATE, ["before finalize"], s.add_pressure_chamber, surf[:3])
    s.set_pressure(1, "constant", p=3.0); s.set_pressure(1, "gas", amount=2.0, ambient=0.5)      # and after
    msg = _raises(pkg, ERR_ARG, ["chamber 2", "closed", "edge ("], s.set_pressure, 2, "gas", amount=1.0, ambient=1.0)
    assert _named_edge(msg) <= set(int(v) for v in surf[hole])
    _raises(pkg, ERR_ARG, ["chamber 3", "have 3"], s.set_pressure, 3, "constant", p=1.0)
    _raises(pkg, ERR_ARG, ["chamber -1"], s.set_pressure, -1, "constant", p=1.0)
    _raises(pkg, ERR_ARG, ["chamber 0", "p inf"], s.set_pressure, 0, "constant", p=float("inf"))
    _raises(pkg, ERR_ARG, ["chamber 0", "mode 2"], s.set_pressure, 0, 2)
    _raises(pkg, ERR_STATE, ["chamber 1", "host-only", "device_id -1"], s.chamber_state, 1)
    _raises(pkg, ERR_ARG, ["chamber 5"], s.chamber_state, 5)
    # inward normals: closed, so add takes it; the rest volume is negative, so initialize refuses
    s2 = pkg.make_bar_system(2, 2, 3, device_id=-1)
    assert s2.add_pressure_chamber(surf[:2]) == 0
    assert s2.add_pressure_chamber(surf[:, [0, 2, 1]], "gas", amount=1.0, ambient=1.0) == 1
    _raises(pkg, ERR_ARG, ["chamber 1", "rest volume", "-0.0015"], s2.initialize)
    for bad in (dict(dt=0.0), dict(mode=5), dict(p=float("nan")), dict(tris=[[0, 1, 9]]), dict(tris=np.zeros((0, 3), np.int32))):
        ch = dict(tris=bad.get("tris", [[0, 1, 2]]), mode=bad.get("mode", "constant"), p=bad.get("p", 1.0))
        with pytest.raises(pkg.AdmmHipError):
            pkg.pressure_query(np.eye(3), np.ones(3), [ch], bad.get("dt", DT))


def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    import os
    assert os.path.exists(compile_cpp("pressure", pkg))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the scene of the bitwise tests
# ---------------------------------------------------------------------------------------------------------------------------------
BAR_DIMS, BAR_H = (2, 2, 3), 0.05
N_BAR = 36
N_P = 500                       # free particles; the last 11 are in no chamber, particles 400 .. 419 only in the inactive one
N_ALL = N_BAR + N_P
V_BAR = 0.1 * 0.1 * 0.15


def _chambers(pkg):
    """the chambers of the scene, in the order they are added: the bar's k = 0 end face (constant), the bar's closed surface (gas; its
    nodes of the end face are in both), soups of 1, 63, 65, 129 and 16 449 triangles over the particles (constant), a hub fan of 70
    triangles about one particle, a pair of soups over the same twelve particles, one inactive chamber.  Their first triangles sit at
    offsets 0, 8, 72, 73, 136, 201, 330, 16 779, ... of the triangle tables: none but the first a multiple of 64."""
    mg = pkg.meshgen
    xb, tets = mg.bar(*BAR_DIMS, BAR_H)
    surf = mg.tet_surface(tets)
    face = surf[(surf < 9).all(1)]
    assert len(surf) == 64 and len(face) == 8
    rng = np.random.default_rng(4242)
    P = lambda lo, hi: np.arange(N_BAR + lo, N_BAR + hi)
    ch = [dict(tris=face, mode="constant", p=-150.0),
          dict(tris=surf, mode="gas", amount=1.2 * 1000.0 * V_BAR, ambient=1000.0)]
    for k, (nt, p) in enumerate(zip((1, 63, 65, 129, SIZES[-1]), (3.0, -2.0, 1.5, -0.75, 0.5))):
        ch.append(dict(tris=_soup(rng, P(0, 380) if nt > 129 else P(40 * k, 40 * k + 40), nt), mode="constant", p=p))
    ch.append(dict(tris=_fan(rng, N_BAR + 390, P(380, 400), 70), mode="constant", p=2.0))
    ch.append(dict(tris=_soup(rng, P(200, 212), 20), mode="constant", p=1.25))
    ch.append(dict(tris=_soup(rng, P(200, 212), 33), mode="constant", p=-2.5))
    ch.append(dict(tris=_soup(rng, P(395, 420), 40), mode="constant", p=0.0))
    off = np.cumsum([0] + [len(c["tris"]) for c in ch])[:-1]
    assert all(o % 64 for o in off[1:]) and sorted(len(c["tris"]) for c in ch[2:7]) == [1, 63, 65, 129, SIZES[-1]]
    return ch


def _scene(pkg, chambers, stream=None, v0=True):
    """a 2 x 2 x 3 corotational bar (36 nodes: the elimination order is not the caller's) and free particles over a far floor, as in
    tests/test_damping.py, gravity; every node moves: the bar is thrown, spun and bent, the particles fly at random"""
    mg = pkg.meshgen
    xb, tets = mg.bar(*BAR_DIMS, BAR_H)
    assert len(xb) == N_BAR
    rng = np.random.default_rng(2024)
    xp = rng.uniform(1.0, 2.0, (N_P, 3)) + [0.0, 5.0, 0.0]
    x = np.concatenate([xb, xp])
    m = np.concatenate([mg.lumped_tet_mass(xb, tets, 1000.0), rng.uniform(0.5, 2.0, N_P)])
    s = pkg.System(device_id=0, stream=stream)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [1e5])
    s.add_forces(KIND["COLLISION"], np.arange(N_BAR, N_ALL, dtype=np.int32), [8.0])
    s.add_gravity(G)
    s.set_collision_shapes([FLOOR], [[0.0, -100.0, 0.0, 0.0]])
    s.cid = [s.add_pressure_chamber(**c) for c in (chambers or [])]
    s.initialize()
    if v0:
        c = xb.mean(0)
        vb = [0.3, 0.5, -0.2] + np.cross([1.0, -2.0, 0.5], xb - c) + 0.5 * np.sin(40.0 * xb[:, [2, 0, 1]])
        s.m_v = np.concatenate([vb, rng.normal(size=(N_P, 3))]).ravel()
    s.m = m
    return s


def _xv(s):
    return s.m_x.reshape(-1, 3).copy(), s.m_v.reshape(-1, 3).copy()


def _same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in FIELDS)


def _frame(pkg, A, B, chambers, iters=10):
    """one frame of the chamber-less A and the loaded B from the same state: A's v is B's plus the twin's dv on that state (the load
    touches nothing else of the solver's state); asserts B's x and v against A's, bit for bit; -> the twin's dv"""
    x, v = _xv(B)
    assert np.array_equal(A.m_x.reshape(-1, 3), x)
    dv, _ = pkg.pressure_query(x, B.m, chambers, DT)
    A.m_v = (v + dv).ravel()
    A.step(iters); B.step(iters)
    xa, va = _xv(A); xb, vb = _xv(B)
    assert np.array_equal(xb, xa) and np.array_equal(vb, va)
    return dv


@pytest.mark.gpu
def test_same_bits_as_the_twin(pkg):
    """A without chambers and v0 + dv from pressure_query, B with the chambers and v0, C without chambers and v0: after one frame of 10
    iterations B's x and v are A's bit for bit; every active chamber moved its nodes (B against C), and the particles in no active
    chamber did not (they are free, so nothing couples them to the loaded ones).  chamber_state of every chamber, the inactive one
    included, is the twin's record field by field, bit for bit, before the first frame and after it; asking changes nothing: x and v
    read the same afterwards, and the frame that follows the first asking is the one compared with A."""
    chambers = _chambers(pkg)
    A, B, C = _scene(pkg, None), _scene(pkg, chambers), _scene(pkg, None)
    x0, v0 = _xv(B)
    _, recs = pkg.pressure_query(x0, B.m, chambers, DT)
    for c, r in zip(B.cid, recs):
        assert _same_record(B.chamber_state(c), r), c
        assert r["collapsed"] == 0 and r["n_tris"] == len(chambers[c]["tris"])
    assert recs[1]["pressure"] > 0 and abs(recs[1]["volume"] - V_BAR) < 1e-12
    assert np.array_equal(B.m_x.reshape(-1, 3), x0) and np.array_equal(B.m_v.reshape(-1, 3), v0)
    dv = _frame(pkg, A, B, chambers)
    C.step(10)
    xb, vb = _xv(B); xc, vc = _xv(C)
    in_active = np.zeros(N_ALL, bool)
    for ch in chambers:
        nodes = np.unique(ch["tris"])
        if _active(ch):
            in_active[nodes] = True
            assert dv[nodes].any(1).all(), "every node of an active chamber is pushed"
            assert not np.array_equal(vb[nodes], vc[nodes]) and not np.array_equal(xb[nodes], xc[nodes])
    out = ~in_active
    out[:N_BAR] = False
    assert out.sum() >= 11 + 20 and not dv[out].any()
    assert np.array_equal(vb[out], vc[out]) and np.array_equal(xb[out], xc[out])
    _, recs = pkg.pressure_query(xb, B.m, chambers, DT)
    for c, r in zip(B.cid, recs):
        assert _same_record(B.chamber_state(c), r), c
    assert np.array_equal(B.m_x.reshape(-1, 3), xb) and np.array_equal(B.m_v.reshape(-1, 3), vb)


@pytest.mark.gpu
def test_off_is_off(pkg):
    """no chamber, chambers that are all inactive, and pressures set and then taken back before the first frame, against a context
    built without the calls, over 5 frames: x, v and graph_state() identical; asking an inactive chamber for its state works and
    changes nothing"""
    chambers = _chambers(pkg)
    off = [dict(tris=c["tris"], mode=c["mode"], p=0.0, amount=0.0, ambient=0.0) for c in chambers]
    plain, none, zero, reset = _scene(pkg, None), _scene(pkg, []), _scene(pkg, off), _scene(pkg, chambers)
    for c, o in zip(reset.cid, off):
        reset.set_pressure(c, **{k: v for k, v in o.items() if k != "tris"})
    for frame in range(5):
        for s in (plain, none, zero, reset):
            s.step(10)
        if frame == 2:
            st = zero.chamber_state(zero.cid[6])
            assert st["n_tris"] == SIZES[-1] and st["area"] > 0 and st["pressure"] == 0.0
        for s in (none, zero, reset):
            assert np.array_equal(s.m_x, plain.m_x) and np.array_equal(s.m_v, plain.m_v), frame
    assert none.graph_state() == zero.graph_state() == reset.graph_state() == plain.graph_state()


@pytest.mark.gpu
def test_launch_modes(pkg, monkeypatch):
    """the scene under ADMM_HIP_GRAPH=0, under the default (the iteration graph and, from the second frame with the same count on, the
    frame graph: asserted) and on a caller's non-blocking stream: x and v after three frames are the same bits in all three"""
    from checkers import nonblocking_stream
    chambers = _chambers(pkg)
    out = {}
    for mode in ("eager", "default", "stream"):
        if mode == "eager":
            monkeypatch.setenv("ADMM_HIP_GRAPH", "0")
        else:
            monkeypatch.delenv("ADMM_HIP_GRAPH", raising=False)
        st = nonblocking_stream()[0] if mode == "stream" else None
        s = _scene(pkg, chambers, stream=st.cuda_stream if st else None)
        for _ in range(3):
            s.step(10)
        gs = s.graph_state()
        assert (mode != "eager" or gs["graph_launches"] == 0) and (mode != "default" or gs["frame_graph_iters"] == 10), (mode, gs)
        out[mode] = (s.m_x, s.m_v)
    for mode in ("default", "stream"):
        assert np.array_equal(out[mode][0], out["eager"][0]) and np.array_equal(out[mode][1], out["eager"][1]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["residuals", "tolerance", "acceleration", "keep_z_off", "set_pressure"])
def test_the_solvers_options_do_not_matter(pkg, option):
    """residual tracking, a tolerance exit (three of ten iterations: asserted), Anderson acceleration with window 3, keep_z off, and
    set_pressure changing modes and parameters between two frames: over three frames B's x and v are A's, A fed the twin's dv and run
    with the same option"""
    chambers = _chambers(pkg)
    A, B = _scene(pkg, None), _scene(pkg, chambers)
    for s in (A, B):
        if option == "residuals":
            s.enable_residuals(True)
        elif option == "tolerance":
            s.set_tolerance(1e300, 1e300, 3)
        elif option == "acceleration":
            s.set_acceleration(3)
        elif option == "keep_z_off":
            s.keep_z(False)
    _frame(pkg, A, B, chambers)
    if option == "tolerance":
        assert B.residuals()[2] == 3
    if option == "set_pressure":      # gas -> constant, new parameters, one chamber switched off, the inactive one switched on
        chambers = [dict(c) for c in chambers]
        chambers[0]["p"] = 80.0
        chambers[1] = dict(tris=chambers[1]["tris"], mode="constant", p=-60.0)
        chambers[4]["p"] = 0.0
        chambers[-1]["p"] = 1.75
        for c in (0, 1, 4, len(chambers) - 1):
            B.set_pressure(c, **{k: v for k, v in chambers[c].items() if k != "tris"})
    _frame(pkg, A, B, chambers)
    if option == "set_pressure":      # and back to the gas law, with another amount
        chambers[1] = dict(tris=chambers[1]["tris"], mode="gas", amount=0.9 * 1000.0 * V_BAR, ambient=1000.0)
        B.set_pressure(1, mode="gas", amount=chambers[1]["amount"], ambient=1000.0)
    dv = _frame(pkg, A, B, chambers)
    assert dv.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: shards
# ---------------------------------------------------------------------------------------------------------------------------------
def _shard_bar(pkg, shard, chambers):
    mg = pkg.meshgen
    x, tets = mg.bar(*BAR_DIMS, BAR_H)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    s = pkg.System(device_id=0)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [1e5])
    top = np.flatnonzero(x[:, 1] == x[:, 1].max())[:2].astype(np.int32)
    s.add_forces(KIND["ANCHOR"], top, [-1.0, 1.0])
    s.add_gravity(G)
    s.cid = [s.add_pressure_chamber(**c) for c in chambers]
    s.set_shard(*shard); s.set_shard_mode("subtree")
    s.m = m
    return s


@pytest.mark.gpu
def test_two_shards(pkg, monkeypatch):
    """two ranks on one GPU (threads and hooks as tests/test_damping.py test_two_shards starts them; a corotational bar hanging from two
    anchors, its surface a gas chamber, its end face a constant one; two frames): every rank applies the load to its own whole copy of
    v, so both ranks' x and v are the same bits, and each rank's equal those of a chamber-less sharded run of the same frame started
    from v + dv, dv the twin's on the loaded ranks' state"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "8")
    world = 2
    chambers = _chambers(pkg)[:2]
    runs = {}
    for name, chs in (("plain", []), ("loaded", chambers)):
        shards = [_shard_bar(pkg, (r, world), chs) for r in range(world)]
        for sh, hk in zip(shards, _thread_allreduce_hooks(world)):
            sh.set_allreduce(hk)
        pkg.initialize_together(shards)
        runs[name] = shards

    def step_all(shards):
        errs = []

        def run(r):
            try:
                shards[r].step(10)
            except Exception as e:  # noqa: BLE001
                errs.append((r, e))
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not errs, errs

    for frame in range(2):
        for r in range(world):
            x, v = _xv(runs["loaded"][r])
            dv, _ = pkg.pressure_query(x, runs["loaded"][r].m, chambers, DT)
            assert dv.any(1).sum() == len(np.unique(chambers[1]["tris"])) == 34      # (the bar's two inner nodes are on no surface)
            runs["plain"][r].m_v = (v + dv).ravel()
        step_all(runs["plain"]); step_all(runs["loaded"])
        l0x, l0v = _xv(runs["loaded"][0])
        for r in range(world):
            xa, va = _xv(runs["plain"][r]); xb, vb = _xv(runs["loaded"][r])
            assert np.array_equal(xb, xa) and np.array_equal(vb, va), (frame, r)
            assert np.array_equal(vb, l0v) and np.array_equal(xb, l0x), (frame, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: what it is for
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_bar_inflates_and_keeps_its_momentum(pkg):
    """a free corotational 2 x 2 x 6 bar, no gravity, at rest, its surface a gas chamber with ambient = p0 and amount = 2 p0 V0 (a gauge
    pressure of p0 at rest), 20 frames of 10 iterations.  chamber_state at the start of every frame: V lies above V0 from the second
    frame on, and the last frame's gauge pressure below the first frame's.  The global solve conserves linear momentum for
    difference-operator elements (D 1 = 0) and a closed chamber adds none, so |sum m v| / sum m |v| per frame is compared with the same
    ratio of a chamber-less run of the same bar started from the first frame's dv as its v -- the existing code path only.  The margin
    is twice that run's largest ratio, for run-to-run rounding; it is measured here, not invented.  Measured on the MI355X: DESIGN.md
    section 3."""
    mg = pkg.meshgen
    x, tets = mg.bar(2, 2, 6, BAR_H)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    surf = mg.tet_surface(tets)
    V0, p0 = 0.1 * 0.1 * 0.3, 2000.0
    chamber = dict(tris=surf, mode="gas", amount=2.0 * p0 * V0, ambient=p0)

    def build(chambers):
        s = pkg.System(device_id=0)
        s.set_timestep(DT)
        s.add_nodes(x.ravel(), np.repeat(m, 3))
        s.add_forces(KIND["TET_LINEAR"], tets, [1e5])
        cid = [s.add_pressure_chamber(**c) for c in chambers]
        s.initialize()
        return s, cid

    def ratio(s):
        v = s.m_v.reshape(-1, 3)
        return float(np.linalg.norm((m[:, None] * v).sum(0)) / (m * np.linalg.norm(v, axis=1)).sum())

    s, cid = build([chamber])
    states, loaded = [], []
    for frame in range(20):
        states.append(s.chamber_state(cid[0]))
        s.step(10)
        loaded.append(ratio(s))
    dv, _ = pkg.pressure_query(x, m, [chamber], DT)
    q, _ = build([])
    q.m_v = dv.ravel()
    plain = []
    for frame in range(20):
        q.step(10)
        plain.append(ratio(q))
    V = np.array([st["volume"] for st in states]); P = np.array([st["pressure"] for st in states])
    print("inflating bar: V0 %.6e, V per frame / V0: %s" % (V0, " ".join("%.4f" % (v / V0) for v in V)))
    print("inflating bar: gauge pressure, first frame %.6e, last frame %.6e (p0 = %g)" % (P[0], P[-1], p0))
    print("inflating bar: |sum m v| / sum m |v|, largest over 20 frames: loaded %.3e, chamber-less %.3e -> margin %.3e" % (max(loaded), max(plain), 2.0 * max(plain)))
    assert abs(V[0] - V0) <= 1e-12 * V0 and abs(P[0] - p0) <= 1e-9 * p0
    assert (V[1:] > V0).all() and P[-1] < P[0]
    assert all(st["collapsed"] == 0 for st in states)
    assert max(loaded) <= 2.0 * max(plain), (max(loaded), max(plain))


# ---------------------------------------------------------------------------------------------------------------------------------
# the C++ class mirror (host/admm/System.hpp): tests/cpp/pressure.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cpp_mirror_loads(pkg):
    """System::add_pressure_chamber, set_pressure and chamber_state on nine particles with a gas tetrahedron and a constant flap that
    share a particle: the program prints the start state, the records chamber_state gives there, the increment it handed to a
    chamber-less system, and both systems after one step, all with %.17g; the records and the increment must be pressure_query's and the
    loaded system's x and v the chamber-less one's, in every printed digit (which are all of them)"""
    import subprocess
    from test_cpp_host import compile_cpp
    r = subprocess.run([compile_cpp("pressure", pkg)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = {}
    for line in r.stdout.splitlines():
        key, rest = line.split(":", 1)
        rows.setdefault(key, []).append([float(t) for t in rest.split()])
    start = np.array(rows["start"])                                       # node, m, x[3], v[3]
    m, x = start[:, 1], start[:, 2:5]
    laws = rows["law"]
    assert [int(l[0]) for l in laws] == [pkg.PRESSURE["GAS"], pkg.PRESSURE["CONSTANT"]]
    chambers = [dict(tris=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], mode="gas", amount=laws[0][1], ambient=laws[0][2]),
                dict(tris=[[3, 4, 5], [5, 6, 7]], mode="constant", p=laws[1][1])]
    dv, recs = pkg.pressure_query(x, m, chambers, DT)
    assert np.array_equal(np.array(rows["dv"])[:, 1:], dv) and dv[:8].any(1).all() and not dv[8].any()
    for row, rec in zip(rows["record"], recs):
        flat = np.concatenate([[rec["volume"], rec["area"]], rec["area_vector"], [rec["pressure"]], rec["resultant"], [rec["n_tris"], rec["collapsed"]]])
        assert np.array_equal(np.array(row), flat), (row, flat)
    assert recs[0]["volume"] > 0 and recs[0]["pressure"] != 0.0
    plain, loaded = np.array(rows["plain"]), np.array(rows["loaded"])
    assert np.array_equal(plain, loaded) and not np.array_equal(loaded[:, 1:4], x)
