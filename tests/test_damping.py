"""Velocity damping per node group (include/admm_hip.h "velocity damping per node group"; csrc/damping.hpp, kernels_damping.hpp,
abi_damping.inc, damping_host.cpp).

CPU: damping_query against a numpy.longdouble restatement of the rule to a bound derived from the summation tree, the exact
identities of the filter, degenerate groups, and the errors a host-only context can show.
GPU: the device's v and moments against the host twin bit for bit (groups of 1 .. 16 449 nodes at offsets that are no multiples of 64,
through a permuted node order), off is off, the launch modes, the solver's options, two shards, a spinning bar, the C++ class mirror.

The rounding bound.  A group's sum runs through a fixed tree: the wave butterfly (6 additions on the way to lane 0), the reducer's
strided loop (ceil(partials / 256) additions) and its LDS fold (8), so a sum of n terms carries at most D = 6 + ceil(nb / 256) + 8
roundings on any path, nb = ceil(n / 64), plus the k roundings of a term itself: |computed - exact| <= gamma(D + k) sum |term|, gamma as
in Higham.  Everything below propagates that through the rule to first order, with the errors of c and v_c carried into pass 2, and the
solve's error through the conditioning of I:  |d omega| <= |I^-1| (|dL| + |dI| |omega|) + the adjugate's own roundings, which are
gamma(7) 3 (F^2 |L| + F^3 |omega|) / det with F = |I|_F (a product and a difference per adjugate entry, three products and two sums
per row and for the determinant, one division; every adjugate entry is bounded by F^2)."""
import threading

import numpy as np
import pytest

from checkers import EPS, KIND, gamma

L = np.longdouble
DT = 0.04
G = np.array([0.0, -9.8, 0.0])
FLOOR = 0
ERR_ARG, ERR_HIP, ERR_STATE = 1, 2, 3
SIZES = [1, 2, 3, 63, 64, 65, 129, 257 * 64 + 1]      # the last: 257 full blocks and one node, the reducer's strided loop wraps
FIELDS = ("mass", "com", "p", "l", "inertia", "omega", "t_total", "t_rigid", "n_nodes", "degenerate")
DEGENERATE = 1e-10                                     # DAMPING_DEGENERATE (csrc/damping.hpp)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule in long double, with its error bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _depth(n):
    nb = (n + 63) // 64
    return 6 + (nb + 255) // 256 + 8


def _abscross(a, b):
    """|a| x |b| with every minus a plus: the magnitude a rounded cross product's error is measured against"""
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _sym(i6):
    xx, yy, zz, xy, xz, yz = i6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=L)


def _reference(m, x, v, dt, drag, internal):
    """-> (values, bounds): the rule of csrc/damping.hpp in long double and the first-order rounding bound of the double evaluation
    (module docstring), per field of the moments record and for v_out"""
    m, x, v = L(m), L(x), L(v)
    n = len(m)
    u, D = L(EPS), _depth(n)
    M = m.sum(); S = (m[:, None] * x).sum(0); P = (m[:, None] * v).sum(0)
    Ti = L(0.5) * m * (v * v).sum(1); T = Ti.sum()
    c, vc = S / M, P / M
    e_M = gamma(D) * M
    e_S = gamma(D + 1) * (m[:, None] * np.abs(x)).sum(0)
    e_P = gamma(D + 1) * (m[:, None] * np.abs(v)).sum(0)
    e_T = gamma(D + 6) * Ti.sum()
    e_c = (e_S + np.abs(S) * e_M / M) / M + u * np.abs(c)
    e_vc = (e_P + np.abs(P) * e_M / M) / M + u * np.abs(vc)
    r, w = x - c, v - vc
    dr, dw = e_c + u * np.abs(r), e_vc + u * np.abs(w)
    Li = m[:, None] * np.cross(r, w)
    Lsum = Li.sum(0)
    e_L = (m[:, None] * (_abscross(dr, w) + _abscross(r, dw) + gamma(3) * _abscross(r, w))).sum(0) + gamma(D) * (m[:, None] * _abscross(r, w)).sum(0)
    r2 = r * r
    It = np.stack([m * (r2[:, 1] + r2[:, 2]), m * (r2[:, 0] + r2[:, 2]), m * (r2[:, 0] + r2[:, 1]), -m * r[:, 0] * r[:, 1], -m * r[:, 0] * r[:, 2], -m * r[:, 1] * r[:, 2]], 1)
    ar = np.abs(r)
    dIt = np.stack([2 * m * (ar[:, 1] * dr[:, 1] + ar[:, 2] * dr[:, 2]), 2 * m * (ar[:, 0] * dr[:, 0] + ar[:, 2] * dr[:, 2]), 2 * m * (ar[:, 0] * dr[:, 0] + ar[:, 1] * dr[:, 1]),
                    m * (ar[:, 0] * dr[:, 1] + dr[:, 0] * ar[:, 1]), m * (ar[:, 0] * dr[:, 2] + dr[:, 0] * ar[:, 2]), m * (ar[:, 1] * dr[:, 2] + dr[:, 1] * ar[:, 2])], 1)
    I6 = It.sum(0)
    e_I = (dIt + gamma(3) * np.abs(It)).sum(0) + gamma(D) * np.abs(It).sum(0)
    I = _sym(I6)
    det = I[0, 0] * (I[1, 1] * I[2, 2] - I[1, 2] ** 2) - I[0, 1] * (I[0, 1] * I[2, 2] - I[0, 2] * I[1, 2]) + I[0, 2] * (I[0, 1] * I[1, 2] - I[0, 2] * I[1, 1])
    tr3 = (I6[0] + I6[1] + I6[2]) / 3
    degenerate = int(n < 3 or not det > L(DEGENERATE) * tr3 ** 3)
    if degenerate:
        om, e_om = np.zeros(3, L), L(0.0)
    else:
        adj = np.array([[I[1, 1] * I[2, 2] - I[1, 2] ** 2, I[0, 2] * I[1, 2] - I[0, 1] * I[2, 2], I[0, 1] * I[1, 2] - I[0, 2] * I[1, 1]],
                        [0, I[0, 0] * I[2, 2] - I[0, 2] ** 2, I[0, 1] * I[0, 2] - I[0, 0] * I[1, 2]],
                        [0, 0, I[0, 0] * I[1, 1] - I[0, 1] ** 2]], dtype=L)
        adj = adj + np.triu(adj, 1).T
        om = adj @ Lsum / det
        lam = np.linalg.eigvalsh(np.asarray(I, dtype=np.float64))
        inv_norm = L(1.0 / lam.min()) * (1 + L(1e-6))                        # |I^-1|_2 (the eigenvalues in double: six digits are plenty for a bound)
        F = np.sqrt((I * I).sum())
        nrm = lambda a: np.sqrt((a * a).sum())
        e_I_F = np.sqrt((e_I[:3] ** 2).sum() + 2 * (e_I[3:] ** 2).sum())
        e_om = inv_norm * (nrm(e_L) + e_I_F * nrm(om)) + gamma(7) * 3 * (F ** 2 * nrm(Lsum) + F ** 3 * nrm(om)) / det
    t_rigid = L(0.5) * M * (vc * vc).sum() + L(0.5) * (om * Lsum).sum()
    e_tr = L(0.5) * (e_M * (vc * vc).sum() + 2 * M * (np.abs(vc) * e_vc).sum() + e_om * np.abs(Lsum).sum() + (np.abs(om) * e_L).sum()) + \
        gamma(8) * (L(0.5) * M * (vc * vc).sum() + L(0.5) * (np.abs(om) * np.abs(Lsum)).sum())
    val = dict(mass=M, com=c, p=P, l=Lsum, inertia=I6, omega=om, t_total=T, t_rigid=t_rigid, n_nodes=n, degenerate=degenerate)
    bnd = dict(mass=e_M, com=e_c, p=e_P, l=e_L, inertia=e_I, omega=np.full(3, e_om), t_total=e_T, t_rigid=e_tr)
    # apply: beta and s from the doubles (three and two roundings), v + beta ((v_c + omega x r) - v), then s v
    beta = L(internal) * L(dt) / (1 + L(internal) * L(dt)); s = 1 / (1 + L(drag) * L(dt))
    vo = v.copy(); e_v = np.zeros_like(v)
    if internal > 0:
        tgt = vc + np.cross(om, r)
        vo = v + beta * (tgt - v)
        mag = np.abs(vc) + _abscross(om, r)
        e_v = beta * (e_vc + _abscross(np.full(3, e_om), r) + _abscross(om, dr)) + gamma(3 + 5) * (beta * (mag + np.abs(v)) + np.abs(v))
    if internal > 0 or drag > 0:
        vo = s * vo
        e_v = s * e_v + gamma(3) * np.abs(vo)
    val["v_out"], bnd["v_out"] = vo, e_v
    val["beta"] = beta
    return val, bnd


def _state(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, n), rng.normal(size=(n, 3)) + [0.5, -0.3, 0.2], rng.normal(size=(n, 3)) + [0.1, 0.2, -0.1]


def _cube():
    x = np.array([[i, j, k] for i in (0.0, 1.0) for j in (0.0, 1.0) for k in (0.0, 1.0)])
    m = np.array([1.0, 1.5, 0.75, 2.0, 1.25, 1.0, 0.5, 1.75])
    return m, x


def _well_conditioned(mo):
    """far from the degenerate threshold on either side: det I / (tr I / 3)^3 is at least 1e-4 (or the group is degenerate by count / exactly)"""
    I = np.asarray(_sym(mo["inertia"]), dtype=np.float64)
    return np.linalg.det(I) >= 1e-4 * (np.trace(I) / 3) ** 3


def _same_record(a, b):
    return all(np.array_equal(a[k], b[k]) for k in FIELDS)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_damping_query_against_long_double(pkg, n):
    """every field of the moments record and v_out within the bound of the module docstring: gamma(D + k) sum |terms| for the sums, D = 6
    + ceil(nb / 256) + 8 (n = 16 449: D = 16), carried through c, v_c, the terms of pass 2 and, for omega, the conditioning of I; the
    bound is first order in EPS and is not fitted to the result (the largest ratio seen is printed)"""
    m, x, v = _state(n, 100 + n)
    worst = 0.0
    for drag, internal in ((0.7, 6.0), (0.0, 6.0), (0.7, 0.0)):
        vo, mo = pkg.damping_query(m, x, v, DT, drag, internal)
        val, bnd = _reference(m, x, v, DT, drag, internal)
        assert mo["n_nodes"] == n and mo["degenerate"] == val["degenerate"] == int(n < 3)
        assert n < 3 or _well_conditioned(mo)
        for k in ("mass", "com", "p", "l", "inertia", "omega", "t_total", "t_rigid", "v_out"):
            got = L(vo) if k == "v_out" else L(mo[k])
            err, b = np.abs(got - val[k]), bnd[k] + L(2.0) ** -1074
            assert (err <= b).all(), (n, k, err, b)
            worst = max(worst, float((err / b).max()))
        assert np.isfinite(vo).all()
    print("damping_query, %d nodes: depth %d, max error / bound = %.3f" % (n, _depth(n), worst))


def test_exact_identities(pkg):
    """internal = 0: v_out = s v bit for bit; both rates 0: v_out is v; a rigid motion of a cube's corners is a fixed point of the
    internal filter, P and L about c are unchanged by it and T - t_rigid falls by (1 - beta)^2, each within the bound of
    test_damping_query_against_long_double for the quantities involved (the sums' bounds before and after, and the nodes' v_out bounds
    carried into the sums)"""
    for n in (3, 65, 1000):
        m, x, v = _state(n, 7 + n)
        for drag in (0.3, 25.0):
            vo, _ = pkg.damping_query(m, x, v, DT, drag, 0.0)
            assert np.array_equal(vo, (1.0 / (1.0 + drag * DT)) * v)
        vo, _ = pkg.damping_query(m, x, v, DT, 0.0, 0.0)
        assert vo.tobytes() == v.tobytes()
        # momentum, angular momentum, and the energy of what is not rigid motion
        internal = 9.0
        vo, mo = pkg.damping_query(m, x, v, DT, 0.0, internal)
        _, mo2 = pkg.damping_query(m, x, vo, DT, 0.0, 0.0)
        val, bnd = _reference(m, x, v, DT, 0.0, internal)
        val2, bnd2 = _reference(m, x, vo, DT, 0.0, 0.0)
        mm = L(m)[:, None]
        carried_p = (mm * bnd["v_out"]).sum(0)
        carried_l = (mm * _abscross(L(x) - val["com"], bnd["v_out"])).sum(0)
        assert (np.abs(L(mo2["p"]) - L(mo["p"])) <= bnd["p"] + bnd2["p"] + carried_p).all()
        assert (np.abs(L(mo2["l"]) - L(mo["l"])) <= bnd["l"] + bnd2["l"] + carried_l).all()
        beta = val["beta"]
        carried_t = (mm * np.abs(L(vo)) * bnd["v_out"]).sum() * 2       # T and, by Cauchy-Schwarz, t_rigid move by at most sum m |v| |dv| each
        lhs = L(mo2["t_total"]) - L(mo2["t_rigid"])
        rhs = (1 - beta) ** 2 * (L(mo["t_total"]) - L(mo["t_rigid"]))
        tol = bnd2["t_total"] + bnd2["t_rigid"] + bnd["t_total"] + bnd["t_rigid"] + carried_t
        assert abs(lhs - rhs) <= tol, (n, lhs, rhs, tol)
        assert tol <= 1e-9 * L(mo["t_total"]) and (n < 65 or rhs > 0.1 * L(mo["t_total"]) * (1 - beta) ** 2)      # the check binds: the jiggle carries a good part of T
    m, x = _cube()
    a, b, c0 = np.array([0.3, -0.2, 0.1]), np.array([0.5, 1.0, -0.7]), np.array([0.2, 0.1, 0.4])
    v = a + np.cross(b, x - c0)
    vo, mo = pkg.damping_query(m, x, v, DT, 0.0, 12.0)
    _, bnd = _reference(m, x, v, DT, 0.0, 12.0)
    assert mo["degenerate"] == 0 and _well_conditioned(mo)
    assert (np.abs(L(vo) - L(v)) <= bnd["v_out"]).all()
    assert (np.abs(L(mo["omega"]) - L(b)) <= bnd["omega"] + 4 * EPS * np.abs(b).max()).all()      # (v itself was rounded from a, b, c0: two roundings per component)


def test_degenerate_groups(pkg):
    """one node, two nodes, and five nodes on the x axis at exactly representable coordinates (r_y = r_z = 0 exactly, so I_xx and every
    product of inertia are exactly 0 and det I is exactly 0): flagged, omega = 0, every output finite, the target velocity is v_c alone;
    the cube is not flagged"""
    rng = np.random.default_rng(3)
    line = np.zeros((5, 3)); line[:, 0] = [0.0, 0.5, 1.0, 1.5, 4.0]
    for x in (rng.normal(size=(1, 3)), rng.normal(size=(2, 3)), line):
        n = len(x)
        m = np.array([1.0, 2.0, 0.5, 1.0, 1.5])[:n]
        v = rng.normal(size=(n, 3))
        vo, mo = pkg.damping_query(m, x, v, DT, 0.5, 8.0)
        assert mo["degenerate"] == 1 and not mo["omega"].any() and mo["n_nodes"] == n
        assert np.isfinite(vo).all() and all(np.isfinite(mo[k]).all() for k in FIELDS)
        if n == 5:
            I = mo["inertia"]
            assert I[0] == 0.0 and not I[3:].any() and I[1] == I[2] > 0.0
        beta, s = (8.0 * DT) / (1.0 + 8.0 * DT), 1.0 / (1.0 + 0.5 * DT)
        vc = mo["p"] / mo["mass"]
        assert np.abs(vo - s * (v + beta * (vc - v))).max() <= 8 * EPS * np.abs(v).max()
    m, x = _cube()
    _, mo = pkg.damping_query(m, x, rng.normal(size=(8, 3)), DT, 0.5, 8.0)
    assert mo["degenerate"] == 0 and _well_conditioned(mo)


def _raises(pkg, code, words, fn, *a, **k):
    with pytest.raises(pkg.AdmmHipError) as e:
        fn(*a, **k)
    msg = str(e.value)
    assert int(msg.split("error ")[1].split(":")[0]) == code, msg
    for w in words:
        assert w in msg, (w, msg)


def test_errors_on_a_host_only_context(pkg):
    """every refusal names the offending value: a range outside the nodes, node_count < 1, an overlap (both groups), a negative or
    non-finite rate; add after initialize is a state error; set_damping on an unknown group; group_moments without a device"""
    s = pkg.make_bar_system(2, 2, 3, device_id=-1)
    n = s.n_nodes
    assert s.add_damping_group(2, 5, 0.5, 3.0) == 0
    _raises(pkg, ERR_ARG, ["[%d, %d)" % (n - 2, n + 3), "%d nodes" % n], s.add_damping_group, n - 2, 5)
    _raises(pkg, ERR_ARG, ["[-1, 2)"], s.add_damping_group, -1, 3)
    _raises(pkg, ERR_ARG, ["node_count 0"], s.add_damping_group, 10, 0)
    _raises(pkg, ERR_ARG, ["node_count -4"], s.add_damping_group, 10, -4)
    _raises(pkg, ERR_ARG, ["group 1", "[6, 9)", "group 0", "[2, 7)"], s.add_damping_group, 6, 3)
    _raises(pkg, ERR_ARG, ["drag -0.5"], s.add_damping_group, 10, 2, -0.5, 0.0)
    _raises(pkg, ERR_ARG, ["internal nan"], s.add_damping_group, 10, 2, 0.0, float("nan"))
    _raises(pkg, ERR_ARG, ["drag inf"], s.add_damping_group, 10, 2, float("inf"), 0.0)
    assert s.add_damping_group(7, None, 0.0, 0.0) == 1                     # through the last node; nothing refused above was kept
    _raises(pkg, ERR_ARG, ["group 2", "overlaps group 1"], s.add_damping_group, n - 1, 1)
    s.set_damping(1, 2.0, 0.0)                                              # before finalize
    s.initialize()
    _raises(pkg, ERR_STATE, ["before finalize"], s.add_damping_group, 0, 1)
    s.set_damping(0, 0.0, 1.0)                                              # and after
    _raises(pkg, ERR_ARG, ["group 2", "have 2"], s.set_damping, 2, 0.0, 0.0)
    _raises(pkg, ERR_ARG, ["group -1"], s.set_damping, -1, 0.0, 0.0)
    _raises(pkg, ERR_ARG, ["group 0", "internal -1"], s.set_damping, 0, 0.0, -1.0)
    _raises(pkg, ERR_STATE, ["group 1", "host-only", "device_id -1"], s.group_moments, 1)
    _raises(pkg, ERR_ARG, ["group 5"], s.group_moments, 5)
    with pytest.raises(pkg.AdmmHipError):
        pkg.damping_query(np.ones(2), np.zeros((2, 3)), np.zeros((2, 3)), DT, -1.0, 0.0)
    with pytest.raises(pkg.AdmmHipError):
        pkg.damping_query(np.ones(2), np.zeros((2, 3)), np.zeros((2, 3)), 0.0, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the scene of the bitwise tests
# ---------------------------------------------------------------------------------------------------------------------------------
BAR_DIMS, BAR_H = (2, 2, 3), 0.05
N_BAR = 36
# (node_first, node_count, drag, internal): the bar without its first node, then particle groups of the sizes of the CPU test at
# offsets that are no multiples of 64, with gaps; one group internal only, one drag only, the others both; the last nodes in no group
GROUPS = [(1, 35, 0.4, 5.0), (37, 1, 0.0, 4.0), (41, 2, 0.6, 3.0), (50, 3, 0.0, 7.0), (70, 63, 2.5, 0.0), (140, 64, 0.3, 6.0), (210, 65, 0.0, 9.0), (300, 129, 1.0, 2.0),
          (450, SIZES[-1], 0.8, 4.5)]
N_ALL = 450 + SIZES[-1] + 11
assert all(g[0] % 64 for g in GROUPS) and sorted(g[1] for g in GROUPS[1:]) == SIZES


def _scene(pkg, groups=GROUPS, stream=None, v0=True):
    """a 2 x 2 x 3 corotational bar (36 nodes: the elimination order is not the caller's) and free particles over a far floor, as in
    tests/test_reactions.py, gravity; every node moves: the bar is thrown, spun and bent, the particles fly at random"""
    mg = pkg.meshgen
    xb, tets = mg.bar(*BAR_DIMS, BAR_H)
    assert len(xb) == N_BAR
    rng = np.random.default_rng(2024)
    n_p = N_ALL - N_BAR
    xp = rng.uniform(1.0, 2.0, (n_p, 3)) + [0.0, 5.0, 0.0]
    x = np.concatenate([xb, xp])
    m = np.concatenate([mg.lumped_tet_mass(xb, tets, 1000.0), rng.uniform(0.5, 2.0, n_p)])
    s = pkg.System(device_id=0, stream=stream)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m, 3))
    s.add_forces(KIND["TET_LINEAR"], tets, [1e5])
    s.add_forces(KIND["COLLISION"], np.arange(N_BAR, N_ALL, dtype=np.int32), [8.0])
    s.add_gravity(G)
    s.set_collision_shapes([FLOOR], [[0.0, -100.0, 0.0, 0.0]])
    s.gid = [s.add_damping_group(*g) for g in (groups or [])]
    s.initialize()
    if v0:
        c = xb.mean(0)
        vb = [0.3, 0.5, -0.2] + np.cross([1.0, -2.0, 0.5], xb - c) + 0.5 * np.sin(40.0 * xb[:, [2, 0, 1]])
        s.m_v = np.concatenate([vb, rng.normal(size=(n_p, 3))]).ravel()
    s.m = m
    return s


def _twin(pkg, s_m, x, v, groups):
    """damping_query applied per group to the state (x, v) [n][3] -> v_out, the records"""
    out, recs = v.copy(), []
    for first, count, drag, internal in groups:
        sl = slice(first, first + count)
        out[sl], r = pkg.damping_query(s_m[sl], x[sl], v[sl], DT, drag, internal)
        recs.append(r)
    return out, recs


def _xv(s):
    return s.m_x.reshape(-1, 3), s.m_v.reshape(-1, 3)


def _frame(pkg, A, B, groups, iters=10):
    """one frame of the undamped A and the damped B from the same state (B's v handed to A first: the filter touches nothing else of the
    solver's state); asserts B's x and the nodes outside every group against A's and B's v against the twin on A's state, bit for bit"""
    A.m_v = B.m_v
    A.step(iters); B.step(iters)
    xa, va = _xv(A); xb, vb = _xv(B)
    want, recs = _twin(pkg, B.m, xa, va, groups)
    assert np.array_equal(xb, xa)
    inside = np.zeros(len(xa), bool)
    for first, count, drag, internal in groups:
        inside[first:first + count] = True
    assert np.array_equal(vb[~inside], va[~inside]) and (~inside).sum() >= 11
    assert np.array_equal(vb, want)
    return xa, va, recs


@pytest.mark.gpu
def test_same_bits_as_the_twin(pkg):
    """A without groups, B with GROUPS, one frame from the same state: B's x is A's, B's v is damping_query applied per group to A's
    state, nodes outside every group keep A's v, all bit for bit; every group with a rate moved its nodes' v.  The moments: a context
    without groups has no group to ask, so A's state is handed to B (m_x, m_v) and B's group_moments must be the twin's record of A's
    state field by field, bit for bit -- for every group, the drag-only one (which the filter never sums) included."""
    A, B = _scene(pkg, groups=None), _scene(pkg)
    xa, va, recs = _frame(pkg, A, B, GROUPS)
    vb = B.m_v.reshape(-1, 3)
    for (first, count, drag, internal), r in zip(GROUPS, recs):
        moved = not np.array_equal(vb[first:first + count], va[first:first + count])
        assert moved == (count > 1 or drag > 0.0), first                   # (one node alone is its own rigid motion: internal damping leaves it be)
        assert r["degenerate"] == int(count < 3) and (count < 3 or _well_conditioned(r))
    B.m_x = xa.ravel(); B.m_v = va.ravel()
    for g, r in zip(B.gid, recs):
        assert _same_record(B.group_moments(g), r), g
    assert np.array_equal(B.m_v.reshape(-1, 3), va)                          # asking changes nothing


@pytest.mark.gpu
def test_off_is_off(pkg):
    """no group, and groups whose rates are all zero, against a context built without the calls, over 5 frames: x and v bit for bit;
    asking such a group for its moments works and changes nothing"""
    plain = _scene(pkg, groups=None)
    zero = _scene(pkg, groups=[(g[0], g[1], 0.0, 0.0) for g in GROUPS])
    reset = _scene(pkg)                                                     # rates set, then taken back before the first frame
    for g in reset.gid:
        reset.set_damping(g, 0.0, 0.0)
    for frame in range(5):
        plain.step(10); zero.step(10); reset.step(10)
        if frame == 2:
            mo = zero.group_moments(zero.gid[-1])
            assert mo["n_nodes"] == SIZES[-1] and mo["mass"] > 0
        for s in (zero, reset):
            assert np.array_equal(s.m_x, plain.m_x) and np.array_equal(s.m_v, plain.m_v), frame
    assert zero.graph_state() == plain.graph_state() == reset.graph_state()


@pytest.mark.gpu
def test_launch_modes(pkg, monkeypatch):
    """the scene under ADMM_HIP_GRAPH=0, under the default (the iteration graph and, from the second frame with the same count on, the
    frame graph: asserted) and on a caller's non-blocking stream: v after three frames is the same bits in all three"""
    from checkers import nonblocking_stream
    out = {}
    for mode in ("eager", "default", "stream"):
        if mode == "eager":
            monkeypatch.setenv("ADMM_HIP_GRAPH", "0")
        else:
            monkeypatch.delenv("ADMM_HIP_GRAPH", raising=False)
        st = nonblocking_stream()[0] if mode == "stream" else None
        s = _scene(pkg, stream=st.cuda_stream if st else None)
        for _ in range(3):
            s.step(10)
        gs = s.graph_state()
        assert (mode != "eager" or gs["graph_launches"] == 0) and (mode != "default" or gs["frame_graph_iters"] == 10), (mode, gs)
        out[mode] = (s.m_x, s.m_v)
    for mode in ("default", "stream"):
        assert np.array_equal(out[mode][0], out["eager"][0]) and np.array_equal(out[mode][1], out["eager"][1]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["residuals", "tolerance", "acceleration", "keep_z_off", "set_damping"])
def test_the_solvers_options_do_not_matter(pkg, option):
    """residual tracking, a tolerance exit (three of ten iterations: asserted), Anderson acceleration with window 3, keep_z off, and
    set_damping changing the rates between two frames: each time B's v is the twin on A's state, A having run with the same option"""
    A, B = _scene(pkg, groups=None), _scene(pkg)
    for s in (A, B):
        if option == "residuals":
            s.enable_residuals(True)
        elif option == "tolerance":
            s.set_tolerance(1e300, 1e300, 3)
        elif option == "acceleration":
            s.set_acceleration(3)
        elif option == "keep_z_off":
            s.keep_z(False)
    _frame(pkg, A, B, GROUPS)
    if option == "tolerance":
        assert B.residuals()[2] == 3
    groups = GROUPS
    if option == "set_damping":                                            # internal <-> drag only, a group switched off, one switched on from zero
        groups = [(f, c, i + 0.1, d) for f, c, d, i in GROUPS]
        groups[3] = groups[3][:2] + (0.0, 0.0)
        for g, (f, c, d, i) in zip(B.gid, groups):
            B.set_damping(g, d, i)
    _frame(pkg, A, B, groups)
    _frame(pkg, A, B, groups)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: shards
# ---------------------------------------------------------------------------------------------------------------------------------
SHARD_GROUPS = [(1, 20, 0.5, 6.0), (23, 13, 1.5, 0.0)]


def _shard_bar(pkg, shard, groups):
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
    s.gid = [s.add_damping_group(*g) for g in groups]
    s.set_shard(*shard); s.set_shard_mode("subtree")
    s.m = m
    return s


@pytest.mark.gpu
def test_two_shards(pkg, monkeypatch):
    """two ranks on one GPU (threads and hooks as tests/test_reactions.py test_two_shards_add_up_to_one_rank starts them; a corotational
    bar hanging from two anchors, two frames): every rank filters its own whole copy of v, so both ranks' v are the same bits, and each
    rank's v is the twin applied to the state of an undamped sharded run of the same frame (the second frame starts from the damped
    ranks' v)"""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "8")
    world = 2
    runs = {}
    for name, groups in (("plain", []), ("damped", SHARD_GROUPS)):
        shards = [_shard_bar(pkg, (r, world), groups) for r in range(world)]
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
            runs["plain"][r].m_v = runs["damped"][r].m_v
        step_all(runs["plain"]); step_all(runs["damped"])
        d0x, d0v = _xv(runs["damped"][0])
        for r in range(world):
            xa, va = _xv(runs["plain"][r]); xb, vb = _xv(runs["damped"][r])
            want, _ = _twin(pkg, runs["damped"][r].m, xa, va, SHARD_GROUPS)
            assert np.array_equal(xb, xa) and np.array_equal(vb, want), (frame, r)
            assert np.array_equal(vb, d0v) and np.array_equal(xb, d0x), (frame, r)
            assert not np.array_equal(vb, va)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: what it is for
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_spinning_bar_comes_to_rest_in_its_own_frame(pkg):
    """a free corotational 2 x 2 x 6 bar, no gravity, started with a translation, a rigid spin and a bending perturbation; internal = 10 /s
    against an undamped twin run (the same group with zero rates, so that group_moments can be asked), 20 frames of 10 iterations.
    |P|, |L| and T - t_rigid from group_moments at every frame.  The damped run's T - t_rigid ends below the undamped run's.  Its |L|
    stays within a relative margin of the undamped run's at every frame; the margin is measured here, not invented: the largest
    relative change of the UNDAMPED run's |L| over the frames (what implicit Euler and the truncated ADMM loop do to it on their own),
    that much again for the damped run, doubled for run-to-run rounding.  Measured on the MI355X: DESIGN.md section 3."""
    mg = pkg.meshgen
    x, tets = mg.bar(2, 2, 6, BAR_H)
    m = mg.lumped_tet_mass(x, tets, 1000.0)
    c = (m[:, None] * x).sum(0) / m.sum()
    zrel = (x[:, 2] - x[:, 2].min()) / np.ptp(x[:, 2])
    v0 = [0.2, 0.1, -0.3] + np.cross([1.0, 0.5, 0.2], x - c)
    v0[:, 1] += 0.05 * np.sin(np.pi * zrel)
    hist = {}
    for name, internal in (("undamped", 0.0), ("damped", 10.0)):
        s = pkg.System(device_id=0)
        s.set_timestep(DT)
        s.add_nodes(x.ravel(), np.repeat(m, 3))
        s.add_forces(KIND["TET_LINEAR"], tets, [1e5])
        g = s.add_damping_group(0, None, 0.0, internal)
        s.initialize()
        s.m_v = v0.ravel()
        rows = []
        for frame in range(21):
            if frame:
                s.step(10)
            mo = s.group_moments(g)
            assert mo["degenerate"] == 0
            rows.append((np.linalg.norm(mo["p"]), np.linalg.norm(mo["l"]), mo["t_total"] - mo["t_rigid"]))
        hist[name] = np.array(rows)
    u, d = hist["undamped"], hist["damped"]
    drift = float(np.abs(u[:, 1] - u[0, 1]).max() / u[0, 1])
    margin = 2.0 * drift
    dev = float((np.abs(d[:, 1] - u[:, 1]) / u[:, 1]).max())
    print("spinning bar: undamped |L| drifts by %.3e of itself over 20 frames -> margin %.3e; damped |L| deviates from it by %.3e" % (drift, margin, dev))
    print("spinning bar: T - t_rigid, frame 0: %.3e; frame 20: undamped %.3e, damped %.3e; |P| frame 20 / frame 0: undamped %.12f, damped %.12f"
          % (u[0, 2], u[-1, 2], d[-1, 2], u[-1, 0] / u[0, 0], d[-1, 0] / d[0, 0]))
    assert u[0, 2] > 0 and d[-1, 2] < u[-1, 2]
    assert dev <= margin, (dev, margin)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C++ class mirror (host/admm/System.hpp): tests/cpp/damping.cpp
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles(pkg):
    from test_cpp_host import compile_cpp
    import os
    assert os.path.exists(compile_cpp("damping", pkg))


@pytest.mark.gpu
def test_cpp_mirror_damps(pkg):
    """System::add_damping_group, set_damping and group_moments on twelve particles in three groups: the program steps an undamped
    system (the same groups, zero rates) and a damped one from the same state and prints both with %.17g; the damped v must be
    damping_query on the undamped state and the printed moments its records, in every printed digit (which are all of them)"""
    import subprocess
    from test_cpp_host import compile_cpp
    r = subprocess.run([compile_cpp("damping", pkg)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = {}
    for line in r.stdout.splitlines():
        key, rest = line.split(":", 1)
        rows.setdefault(key, []).append([float(t) for t in rest.split()])
    groups = [tuple(int(v) if k < 2 else v for k, v in enumerate(g)) for g in rows["group"]]      # first, count, drag, internal
    assert len(groups) == 3 and any(g[3] == 0.0 < g[2] for g in groups) and any(g[3] > 0.0 for g in groups)
    pre, post = np.array(rows["pre"]), np.array(rows["post"])             # node, m, x[3], v[3]
    m, x, v = pre[:, 1], pre[:, 2:5], pre[:, 5:8]
    assert np.array_equal(post[:, 2:5], x)
    want, recs = _twin(pkg, m, x, v, groups)
    assert np.array_equal(post[:, 5:8], want) and not np.array_equal(want, v)
    for row, rec in zip(rows["moments"], recs):
        flat = np.concatenate([[rec["mass"]], rec["com"], rec["p"], rec["l"], rec["inertia"], rec["omega"], [rec["t_total"], rec["t_rigid"], rec["n_nodes"], rec["degenerate"]]])
        assert np.array_equal(np.array(row), flat), (row, flat)
