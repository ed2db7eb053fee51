"""Elastic forces and tet stresses from the energies' gradient (admm_hip_batch_gradient & co.; csrc/gradient.hpp, csrc/kernels_gradient.hpp).

CPU, through gradient_query / stress_query (the host evaluation of gradient.hpp, the device's bits):
  1. the exact-derivative kinds against central differences of the long-double restatement of the ENERGY (ld_energy below, written
     from the table in include/admm_hip.h), with a bound computed here; the not-finite cases;
  2. TET_VOLUME and TRI_AREA against a long-double restatement of s (d - p) (never against finite differences: they are projective
     forces, not derivatives), and exactly 0 where the limits are inactive;
  3. known answers; 4. argument checks; 5. a host-only context refuses; 6. the C++ mirror compiles.
GPU: the kernels are bitwise the host twin on supplied rows (7) and on gathered rows, with the corner forces and the node sums in the
documented order (8); forces against differences of energy() and the balance of momentum (9); no side effects (10); shards (11); a
not-finite element (12); the C++ mirror (13).

The inputs, the scenes and D_i x are tests/element_cases.py's, shared with tests/test_energy.py.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from checkers import KIND, KIND_NODES, KIND_ROWS
from element_cases import (BAR, BEND_ALPHA, EVALUATED, G, H, LD, SCALE, SPRING_L, TET_KINDS, TRI_KINDS, _bits, _pkg, _same_bits, _state,
                           bend_inputs, build_system, cloth_mesh, deform, element_dx, inputs, ld_det3, ld_singular_values, mixed_forces,
                           needs_ld, spring_inputs, tet_inputs)

gpu = pytest.mark.gpu
U = 2.0 ** -53                      # unit roundoff of double
EPS_LD = float(np.finfo(LD).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = dict(TET_NH=[1e5, 2e5, 5], TET_STVK=[1e5, 2e5, 5], TET_LINEAR=[4000.0], TET_VOLUME=[4000.0, 0.9, 1.1], TRI_FUNG=[50.0, 0.0, 0.0],
              TRI_STRAIN=[100.0, 0.95, 1.05, 1.0], TRI_AREA=[100.0, 3.0, 0.9, 1.1], SPRING=[300.0], BEND=[20.0], ANCHOR=[-1.0, 1.0])
EXACT = ("TET_NH", "TET_STVK", "TET_LINEAR", "TRI_FUNG", "TRI_STRAIN", "SPRING", "BEND", "ANCHOR")
ALL_KINDS = EVALUATED + ("ANCHOR",)
ANCHOR_T = np.array([0.3, -0.2, 0.5])


# ---------------------------------------------------------------------------------------------------------------------------------
# the long-double restatement of the energies, as in tests/test_energy.py but with anchors (inputs, scenes and D_i x: element_cases)
# ---------------------------------------------------------------------------------------------------------------------------------
def rest_rows_elastic(kind, n):
    rest = np.zeros((n, 12))
    if kind == "SPRING":
        rest[:, 0] = SPRING_L
    if kind == "BEND":
        rest[:, :4] = BEND_ALPHA
    return rest


def host_energy(kind, d):
    return _pkg().energy_query(kind, d, PARAMS[kind], rest_rows_elastic(kind, d.shape[0]), SCALE)


def ld_energy_elastic(kind, d):
    """-> (E, mag) in long double from the table of include/admm_hip.h; mag: the sum of the absolute terms the bound is relative to"""
    par = [LD(v) for v in PARAMS["TET_STVK" if kind == "TET_STVK_ABS" else kind]]
    s = LD(SCALE)
    n = d.shape[0]
    inf = LD(np.inf)
    if kind in TET_KINDS or kind == "TET_STVK_ABS":
        M = np.array(d, dtype=LD).reshape(n, 3, 3).transpose(0, 2, 1)      # M[e][row][col]
        I1 = (M * M).sum((1, 2))
        if kind == "TET_NH":
            mu, lam = par[0], par[1]
            J = ld_det3(M)
            ok = J > 0
            L = np.log(np.where(ok, J * J, LD(1)))
            E = s * (mu / 2 * (I1 - L - 3) + lam / 8 * L * L)
            mag = s * (mu / 2 * (I1 + np.abs(L) + 3) + lam / 8 * L * L)
            return np.where(ok, E, inf), mag
        if kind == "TET_STVK":
            mu, lam = par[0], par[1]
            Cm = np.einsum("eki,ekj->eij", M, M)
            Em = (Cm - np.eye(3, dtype=LD)) / 2
            tr = Em[:, 0, 0] + Em[:, 1, 1] + Em[:, 2, 2]
            E = s * (mu * (Em * Em).sum((1, 2)) + lam / 2 * tr * tr)
            return E, s * I1
        if kind == "TET_STVK_ABS":      # the StVK energy's absolute terms (C_BOUND's comment)
            mu, lam = par[0], par[1]
            Ea = (np.einsum("eki,ekj->eij", np.abs(M), np.abs(M)) + np.eye(3, dtype=LD)) / 2
            tr = Ea[:, 0, 0] + Ea[:, 1, 1] + Ea[:, 2, 2]
            return None, s * (mu * (Ea * Ea).sum((1, 2)) + lam / 2 * tr * tr)
        sv = ld_singular_values(M)
        neg = ld_det3(M) < 0
        if kind == "TET_LINEAR":
            nn = np.ones_like(sv)
        else:      # TetVolume::project: four steps on the singular values
            lmin, lmax = par[1], par[2]
            nn = sv.copy(); dd = np.zeros_like(sv)
            for _ in range(4):
                det = nn[:, 0] * nn[:, 1] * nn[:, 2]
                f = det - np.minimum(np.maximum(det, lmin), lmax)
                g = np.stack([nn[:, 1] * nn[:, 2], nn[:, 0] * nn[:, 2], nn[:, 0] * nn[:, 1]], axis=1)
                sc = -((f - (g * dd).sum(1)) / (g * g).sum(1))
                dd = sc[:, None] * g
                nn = sv + dd
        nn = nn.copy(); nn[neg, 2] = LD(-1)
        return s / 2 * ((sv - nn) ** 2).sum(1), s * I1
    if kind in TRI_KINDS:
        M = np.array(d, dtype=LD).reshape(n, 2, 3).transpose(0, 2, 1)      # [e][row 0..2][col 0..1]
        n2 = (M * M).sum((1, 2))
        if kind == "TRI_FUNG":
            mu = par[0]
            a, b, c = (M[:, :, 0] ** 2).sum(1), (M[:, :, 1] ** 2).sum(1), (M[:, :, 0] * M[:, :, 1]).sum(1)
            g = a * b - c * c
            ok = g > 0
            I1 = n2 + 1 / np.where(ok, g, LD(1))
            ex = np.exp(np.minimum(I1 - 3, LD(5000)))
            ok = ok & (ex < LD(np.finfo(np.float64).max))
            return np.where(ok, s * mu / 2 * (ex - 1), inf), s * (n2 + mu / 2 * (ex * (1 + I1 + 3) + 1))
        sv = ld_singular_values(M)
        if kind == "TRI_STRAIN":
            nn = np.ones_like(sv)
        else:
            iters, lmin, lmax = int(par[1]), par[2], par[3]
            nn = sv.copy(); dd = np.zeros_like(sv)
            for _ in range(iters):
                v = nn[:, 0] * nn[:, 1]
                f = v - np.maximum(np.minimum(v, lmax), lmin)
                g = np.stack([nn[:, 1], nn[:, 0]], axis=1)
                q = -((f - (g * dd).sum(1)) / (g * g).sum(1))
                dd = q[:, None] * g
                nn = sv + dd
        return s / 2 * ((sv - nn) ** 2).sum(1), s * n2
    D = np.array(d, dtype=LD)
    if kind == "SPRING":
        nrm = np.sqrt((D * D).sum(1))
        p = np.where((nrm > 0)[:, None], LD(SPRING_L) * D / np.where(nrm > 0, nrm, LD(1))[:, None], LD(0))
        return s / 2 * ((D - p) ** 2).sum(1), s * ((D * D).sum(1) + LD(SPRING_L) ** 2)
    a0, a1, _, a3 = [LD(v) for v in BEND_ALPHA]
    al = np.array([a0, a3, a1], dtype=LD)      # the row blocks' coefficients
    R = D.reshape(n, 3, 3)                     # [e][row block][coordinate]
    lam = 2 * np.einsum("r,erj->ej", al, R) / (al * al).sum()
    P = R - LD(0.5) * al[None, :, None] * lam[:, None, :]
    return s / 2 * ((R - P) ** 2).sum((1, 2)), s * (D * D).sum(1)


def rest_rows(kind, n):
    if kind == "ANCHOR":
        r = np.zeros((n, 12)); r[:, :3] = ANCHOR_T
        return r
    return rest_rows_elastic(kind, n)


def host_gradient(kind, d):
    return _pkg().gradient_query(kind, d, PARAMS[kind], rest_rows(kind, d.shape[0]), SCALE)


def ld_energy(kind, d):
    """-> (E, mag) in long double; the elastic kinds' restatement, and the anchor's w^2/2 |x - t|^2 (s = w^2)"""
    if kind == "ANCHOR":
        D = np.array(d, dtype=LD); t = ANCHOR_T.astype(LD)
        return LD(SCALE) / 2 * ((D - t) ** 2).sum(1), LD(SCALE) / 2 * ((np.abs(D) + np.abs(t)) ** 2).sum(1)
    return ld_energy_elastic(kind, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact derivatives against central differences in long double
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_inputs(kind):
    """stretched and sheared rows, random ones (seed 1) and, for TET_STVK and TET_LINEAR, inverted ones; away from where the energy is
    not smooth or its derivative is ill-conditioned (the filters are part of the case list: they depend on the inputs alone)"""
    rng = np.random.default_rng(1)
    if kind in TET_KINDS:
        I = np.eye(3)
        hand = [np.diag([1.5, 1.0, 0.8]), np.diag([0.7, 1.2, 1.1]), I + 0.4 * np.eye(3, k=1), I + np.array([[0, 0.3, -0.2], [0, 0, 0.25], [0, 0, 0]]),
                np.diag([1.3, 0.9, 1.0]) @ (I + 0.3 * np.eye(3, k=-1))]
        M = [I + 0.25 * rng.standard_normal((3, 3)) for _ in range(48)] + hand
        if kind in ("TET_STVK", "TET_LINEAR"):
            inv = np.array([[0.9, 0.1, 0.0], [0.0, -1.2, 0.2], [0.1, 0.0, 1.1]])
            M += [inv] + [inv + 0.1 * rng.standard_normal((3, 3)) for _ in range(4)]
        d = np.array([m.T.reshape(9) for m in M])      # element-major rows: column-major 3x3
        Mm = d.reshape(-1, 3, 3).transpose(0, 2, 1)
        J = np.linalg.det(Mm)
        if kind == "TET_NH":
            d = d[J > 0.2]
        if kind == "TET_LINEAR":      # the nearest rotation is smooth where sigma_1 + sign(J) sigma_2 > 0; its derivative grows as 2 / that
            sv = np.linalg.svd(Mm, compute_uv=False)
            d = d[sv[:, 1] + np.sign(J) * sv[:, 2] > 0.2]
        return d
    if kind in TRI_KINDS:
        I = np.array([1.0, 0, 0, 0, 1.0, 0])
        hand = [np.array([1.5, 0, 0, 0, 0.8, 0]), np.array([1.0, 0, 0, 0.4, 1.0, 0]), np.array([0.9, 0.2, 0.1, -0.1, 1.1, 0.3])]
        d = np.vstack([I + 0.2 * rng.standard_normal((48, 6))] + [h[None] for h in hand])
        sv = np.linalg.svd(d.reshape(-1, 2, 3).transpose(0, 2, 1), compute_uv=False)
        return d[sv[:, 1] > 0.3]      # TRI_FUNG's 1 / g^2 and TRI_STRAIN's 1 / sigma_1
    if kind == "SPRING":
        d = spring_inputs()[:48]
        return d[np.linalg.norm(d, axis=1) > 0.2]
    if kind == "BEND":
        return bend_inputs()[:48]
    return ANCHOR_T + 0.3 * rng.standard_normal((16, 3))


C_SVD = 36 * 8


def analytic_rounding(kind, d, g):
    """the rounding of gradient.hpp's formula in double, per element (a bound on the largest entry's error), from the running error of
    its operations with every term taken in absolute value (Higham, Accuracy and Stability, 3.3): K u times the absolute terms, K the
    number of roundings on the longest path, plus the amplification where a difference of products is divided by:
      TET_NH      g = s (mu d + q C), q = (lambda L / 2 - mu) / J.  J and every cofactor C are differences of rounded products: |dJ| <= 5 u
                  Jabs (Jabs: det's terms in absolute value), so L = log(J J) moves by 2 |dJ| / J + u (|L| + 2) and q by
                  [lambda / 2 dL + 3 u (lambda / 2 |L| + mu)] / J + |q| (|dJ| / J + u).  K = 6 on s (mu |d| + |q| Cabs).
      TET_STVK    g = s d S: 16 roundings from d to g on s |d| Sabs, Sabs = 2 mu Eabs + lambda tr Eabs, Eabs = (|d|^T |d| + I) / 2.
      TRI_FUNG    det = a b - c c moves by 5 u (a b + c c) =: ddet; r = 1 / det^2 relatively by 2 ddet / det + 3 u; I1 by 4 u (a + b) + (ddet /
                  det + 2 u) / det, and k = s mu exp(I1 - 3) relatively by that + 4 u.  On the terms |u_i| + (b |u_i| + |c v_i|) r.
      SPRING      g = s (d - L d / |d|): K = 8 on s (|d| + L).     ANCHOR   w^2 (x - t): K = 3 on w^2 (|x| + |t|).
      BEND        g_r = s (d_r - (d_r - a_r lam / 2)), lam = 2 (a . d) / den: the double difference costs 2 u |d_r|; K = 10 on s (|d_r| + |a_r| sum |a| |d| / den).
      TET_LINEAR, TRI_STRAIN   g = s (d - p): the Jacobi SVD is backward stable, p is the polar factor of d + e with |e|_F <= C_SVD u |d|_F (8 u per
                  plane rotation, at most 36 rotations), and the polar factor moves by at most cond |e|, cond = 2 / (sigma_1 + sign(J)
                  sigma_2) for the 3x3 rotation and 1 / sigma_1 for the 3x2 isometry (Higham, Functions of Matrices, Thm 8.9 / 8.10); the
                  recomposition and the difference add 6 u (|d| + |p|)."""
    par, s, n = PARAMS[kind], SCALE, d.shape[0]
    if kind in TET_KINDS:
        M = d.reshape(n, 3, 3).transpose(0, 2, 1)
        A = np.abs(M)
        nF = np.sqrt((M * M).sum((1, 2)))
    if kind == "TET_NH":
        mu, lam = par[0], par[1]
        J = np.linalg.det(M)
        Jabs = np.array([sum(abs(m[0, p[0]] * m[1, p[1]] * m[2, p[2]]) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))) for m in M])
        L = np.log(J * J)
        q = (0.5 * lam * L - mu) / J
        dJ = 5 * U * Jabs
        dL = 2 * dJ / J + U * (np.abs(L) + 2)
        dq = (0.5 * lam * dL + 3 * U * (0.5 * lam * np.abs(L) + mu)) / J + np.abs(q) * (dJ / J + U)
        Cabs = 2 * A.max((1, 2)) ** 2
        return s * (6 * U * (mu * A.max((1, 2)) + np.abs(q) * Cabs) + dq * Cabs)
    if kind == "TET_STVK":
        mu, lam = par[0], par[1]
        Ea = (np.einsum("eki,ekj->eij", A, A) + np.eye(3)) / 2
        Sa = 2 * mu * Ea + lam * np.trace(Ea, axis1=1, axis2=2)[:, None, None] * np.eye(3)
        return 16 * U * s * np.einsum("eik,ekj->eij", A, Sa).max((1, 2))
    if kind == "TRI_FUNG":
        mu = par[0]
        u, v = d[:, :3], d[:, 3:]
        a, b, c = (u * u).sum(1), (v * v).sum(1), (u * v).sum(1)
        det = a * b - c * c
        ddet = 5 * U * (a * b + c * c)
        r = 1 / det ** 2
        dI1 = 4 * U * (a + b) + (ddet / det + 2 * U) / det
        k = s * mu * np.exp(a + b + 1 / det - 3)
        t_u = np.abs(u) + (b[:, None] * np.abs(u) + np.abs(c[:, None] * v)) * r[:, None]
        t_v = np.abs(v) + (a[:, None] * np.abs(v) + np.abs(c[:, None] * u)) * r[:, None]
        amp = np.maximum((b[:, None] * np.abs(u) + np.abs(c[:, None] * v)).max(1), (a[:, None] * np.abs(v) + np.abs(c[:, None] * u)).max(1)) * r * (2 * ddet / det + 3 * U)
        return k * (np.maximum(t_u.max(1), t_v.max(1)) * (dI1 + 10 * U) + amp)
    if kind == "SPRING":
        return 8 * U * s * (np.abs(d).max(1) + SPRING_L)
    if kind == "ANCHOR":
        return 3 * U * s * (np.abs(d) + np.abs(ANCHOR_T)).max(1)
    if kind == "BEND":
        a0, a1, _, a3 = BEND_ALPHA
        al = np.abs(np.array([a0, a3, a1]))
        R = np.abs(d.reshape(n, 3, 3))
        lam = np.einsum("r,erj->ej", al, R) / (al * al).sum()
        return 10 * U * s * (R + al[None, :, None] * lam[:, None, :]).max((1, 2))
    if kind == "TET_LINEAR":
        sv = np.linalg.svd(M, compute_uv=False)
        cond = 2 / (sv[:, 1] + np.sign(np.linalg.det(M)) * sv[:, 2])
        return U * s * (C_SVD * (1 + cond) * nF + 6 * (nF + math.sqrt(3.0)))
    if kind == "TRI_STRAIN":
        M2 = d.reshape(n, 2, 3).transpose(0, 2, 1)
        sv = np.linalg.svd(M2, compute_uv=False)
        nF = np.sqrt((d * d).sum(1))
        return U * s * (C_SVD * (1 + 1 / sv[:, 1]) * nF + 6 * (nF + math.sqrt(2.0)))
    raise ValueError(kind)


def central_differences(kind, d, h):
    """-> (dE/dd by central differences with step h, the largest mag met): long double"""
    D = np.array(d, dtype=LD)
    out = np.zeros(D.shape, dtype=LD); mag = np.zeros(D.shape[0], dtype=LD)
    for r in range(D.shape[1]):
        Dp, Dm = D.copy(), D.copy()
        Dp[:, r] += h; Dm[:, r] -= h
        (Ep, mp), (Em, mm) = ld_energy(kind, Dp), ld_energy(kind, Dm)
        out[:, r] = (Ep - Em) / (2 * h)
        mag = np.maximum(mag, np.maximum(mp, mm))
    return out, mag


@needs_ld
@pytest.mark.parametrize("kind", EXACT)
def test_exact_gradients_against_long_double_differences(kind):
    """|g - FD_h| <= |FD_h - FD_2h| + eps_ld |E| / h + analytic_rounding, per element (largest entry), nothing hand-picked:
      * truncation: FD_h = g + c h^2 + O(h^4), so FD_2h - FD_h = 3 c h^2 + O(h^4): the difference bounds the h^2 term three times over;
      * the restatement's rounding, as the issue sets it: the long-double epsilon times |E| / h (the larger |E| of a difference's two);
      * the host twin's rounding in double: analytic_rounding above.
    h = 2^-8.  The restatement's true rounding is relative to the energy's absolute terms, which exceed |E| (by far for the quadratic
    kinds, whose truncation is zero), times its operation count; at h = 2^-8 that is 1e-19 x 300 / 4e-3 = 1e-14 of those terms at the
    most, below analytic_rounding's own K u of the same terms for every kind, so the stated bound holds without a term for it.  The
    bound's size against |g| is printed and, being second order in h, asserted to stay below h."""
    d = exact_inputs(kind)
    assert d.shape[0] >= 12, (kind, d.shape)
    g = host_gradient(kind, d)
    assert np.isfinite(g).all()
    h = LD(2.0) ** -8
    f1, _ = central_differences(kind, d, h)
    f2, _ = central_differences(kind, d, 2 * h)
    Eabs = np.zeros(d.shape[0], dtype=LD)
    for r in range(d.shape[1]):
        for sgn in (1, -1):
            D = np.array(d, dtype=LD); D[:, r] += sgn * h
            Eabs = np.maximum(Eabs, np.abs(ld_energy(kind, D)[0]))
    trunc = np.abs(f1 - f2).max(1).astype(np.float64)
    rnd = (EPS_LD * Eabs / h).astype(np.float64)
    ana = analytic_rounding(kind, d, g)
    err = np.abs(g.astype(LD) - f1).max(1).astype(np.float64)
    bound = trunc + rnd + ana
    gm = np.abs(g).max(1) + 1e-300
    print("%s: %d elements; largest error / bound %.3g; largest error / |g| %.3g; median bound / |g| %.3g (truncation %.3g, restatement %.3g, analytic %.3g)"
          % (kind, d.shape[0], (err / bound).max(), (err / gm).max(), np.median(bound / gm), np.median(trunc / gm), np.median(rnd / gm), np.median(ana / gm)))
    assert (err <= bound).all(), (kind, int((err / bound).argmax()), (err / bound).max())
    assert np.median(bound / gm) < float(h)      # second order in h: a wrong coefficient, an error of order |g|, cannot meet it


def test_not_finite_where_the_energy_is_infinite():
    pkg = _pkg()
    for kind in ("TET_NH", "TRI_FUNG"):
        d = inputs(kind)
        E = host_energy(kind, d)
        g = host_gradient(kind, d)
        bad = np.isnan(g).all(1)
        assert np.array_equal(bad, np.isinf(E)) and bad.sum() >= 1, kind
        assert np.isfinite(g[~bad]).all() and np.array_equal(np.isnan(g).any(1), bad)
        assert (g[bad].view(np.uint64) == np.uint64(0x7FF8000000000000)).all()      # the canonical NaN, whatever produced it
    d = tet_inputs()
    st = pkg.stress_query("TET_NH", d, PARAMS["TET_NH"], SCALE)
    J = np.linalg.det(d.reshape(-1, 3, 3).transpose(0, 2, 1))
    assert np.array_equal(np.isnan(st).all(1), np.isinf(host_energy("TET_NH", d)))
    for kind in ("TET_STVK", "TET_LINEAR", "TET_VOLUME"):      # finite gradients, yet no Cauchy stress for J <= 0
        st = pkg.stress_query(kind, d, PARAMS[kind], SCALE)
        sure = np.abs(J) > 1e-9
        assert np.array_equal(np.isnan(st).all(1)[sure], (J <= 0)[sure]) and np.array_equal(np.isnan(st).any(1), np.isnan(st).all(1)), kind
        assert np.isfinite(pkg.gradient_query(kind, d, PARAMS[kind], None, SCALE)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the projective forces of TET_VOLUME and TRI_AREA
# ---------------------------------------------------------------------------------------------------------------------------------
def ld_svd(A):
    """A [n][m][k] -> U [n][m][k], sv [n][k] descending, V [n][k][k] with A = U diag(sv) V^T, in long double: ld_singular_values' one-sided
    Jacobi with the rotations accumulated in V"""
    A = np.array(A, dtype=LD)
    n, m, k = A.shape
    V = np.broadcast_to(np.eye(k, dtype=LD), (n, k, k)).copy()
    for _ in range(12):
        for p in range(k - 1):
            for q in range(p + 1, k):
                ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                al, be, ga = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
                rot = np.abs(ga) > LD(1e-22) * np.sqrt(al * be)
                gg = np.where(rot, ga, LD(1))
                zeta = (be - al) / (LD(2) * gg)
                t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(LD(1) + zeta * zeta))
                c = LD(1) / np.sqrt(LD(1) + t * t)
                s = c * t
                c = np.where(rot, c, LD(1))[:, None]; s = np.where(rot, s, LD(0))[:, None]
                A[:, :, p] = c * ap - s * aq; A[:, :, q] = s * ap + c * aq
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c * vp - s * vq; V[:, :, q] = s * vp + c * vq
    sv = np.sqrt((A * A).sum(1))
    order = np.argsort(-sv, axis=1)
    sv = np.take_along_axis(sv, order, axis=1)
    A = np.take_along_axis(A, order[:, None, :], axis=2); V = np.take_along_axis(V, order[:, None, :], axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):      # (a zero singular value: its column of U is undefined, and unused)
        return A / sv[:, None, :], sv, V


def ld_newton(kind, sv, neg):
    """the singular values the projection moves to (ld_energy_elastic's steps): TetVolume's four, TriArea's `iters`"""
    par = [LD(v) for v in PARAMS[kind]]
    nn = sv.copy(); dd = np.zeros_like(sv)
    if kind == "TET_VOLUME":
        lmin, lmax = par[1], par[2]
        for _ in range(4):
            det = nn[:, 0] * nn[:, 1] * nn[:, 2]
            f = det - np.minimum(np.maximum(det, lmin), lmax)
            g = np.stack([nn[:, 1] * nn[:, 2], nn[:, 0] * nn[:, 2], nn[:, 0] * nn[:, 1]], axis=1)
            dd = (-((f - (g * dd).sum(1)) / (g * g).sum(1)))[:, None] * g
            nn = sv + dd
        nn = nn.copy(); nn[neg, 2] = LD(-1)
        return nn
    iters, lmin, lmax = int(par[1]), par[2], par[3]
    for _ in range(iters):
        v = nn[:, 0] * nn[:, 1]
        f = v - np.maximum(np.minimum(v, lmax), lmin)
        g = np.stack([nn[:, 1], nn[:, 0]], axis=1)
        dd = (-((f - (g * dd).sum(1)) / (g * g).sum(1)))[:, None] * g
        nn = sv + dd
    return nn


@needs_ld
@pytest.mark.parametrize("kind", ["TET_VOLUME", "TRI_AREA"])
def test_projective_forces_against_long_double(kind):
    """g = s (d - p) = s U diag(delta) V^T, delta = sigma - n(sigma): a (generalised) matrix function of d.  The double SVD is backward
    stable, exact for d + e with |e|_F <= C_SVD u |d|_F (8 u per plane rotation, at most 36 rotations), and such a function moves by
    at most kappa |e|_F, kappa the largest of |d delta / d sigma| (central differences in long double), |delta_i - delta_j| / |sigma_i -
    sigma_j| and |delta_i + delta_j| / (sigma_i + sigma_j) (the divided differences that govern U and V: Lewis & Sendov 2005 for
    symmetric functions of singular values).  The Newton steps, the recomposition and the difference add 40 u (|d| + |p|).  So
        |g - g_ld| <= u s [C_SVD (1 + kappa) |d|_F + 40 (|d|_F + |p|_F)]        per element, Frobenius norm.
    Elements whose singular values are closer than 1e-3 to each other or to zero are left out (kappa is not defined there): the
    conditioning of the SVD's vectors, not of the force.  No finite differences: this force is not the energy's derivative."""
    d = inputs(kind)
    n = d.shape[0]
    tet = kind == "TET_VOLUME"
    M = (d.reshape(n, 3, 3) if tet else d.reshape(n, 2, 3)).transpose(0, 2, 1).astype(LD)
    Um, sv, V = ld_svd(M)
    neg = ld_det3(M) < 0 if tet else np.zeros(n, dtype=bool)
    k = sv.shape[1]
    gap = np.min([np.abs(sv[:, i] - sv[:, j]) for i in range(k) for j in range(i + 1, k)] + [sv[:, k - 1]], axis=0)
    keep = (gap > LD(1e-3))
    assert keep.mean() > 0.9
    nn = ld_newton(kind, sv, neg)
    P = np.einsum("emk,ek,enk->emn", Um, nn, V)
    g_ld = LD(SCALE) * (M - P)
    g = host_gradient(kind, d)
    G = (g.reshape(n, 3, 3) if tet else g.reshape(n, 2, 3)).transpose(0, 2, 1)
    err = np.sqrt(((G.astype(LD) - g_ld) ** 2).sum((1, 2))).astype(np.float64)
    delta = sv - nn
    eh = LD(2.0) ** -30
    kappa = np.zeros(n, dtype=LD)
    for i in range(k):
        sp, sm = sv.copy(), sv.copy()
        sp[:, i] += eh; sm[:, i] -= eh
        dd = ((sp - ld_newton(kind, sp, neg)) - (sm - ld_newton(kind, sm, neg))) / (2 * eh)
        kappa = np.maximum(kappa, np.abs(dd).sum(1))
        for j in range(k):
            if j > i:
                kappa = np.maximum(kappa, np.abs(delta[:, i] - delta[:, j]) / np.maximum(np.abs(sv[:, i] - sv[:, j]), LD(1e-3)))
            kappa = np.maximum(kappa, np.abs(delta[:, i] + delta[:, j]) / np.maximum(sv[:, i] + sv[:, j], LD(1e-3)))
    nd, npn = np.sqrt((M * M).sum((1, 2))), np.sqrt((P * P).sum((1, 2)))
    bound = (U * SCALE * (C_SVD * (1 + kappa) * nd + 40 * (nd + npn))).astype(np.float64)
    print("%s: %d of %d elements; largest error / bound %.3g; largest kappa %.3g" % (kind, keep.sum(), n, (err[keep] / bound[keep]).max(), float(kappa[keep].max())))
    assert (err[keep] <= bound[keep]).all(), (kind, (err[keep] / bound[keep]).max())
    moved = np.sqrt((delta ** 2).sum(1)).astype(np.float64) > 1e-3
    assert (moved & keep).sum() > n // 4 and (np.abs(g[moved & keep]).max(1) > 1e-4 * SCALE).all()      # the limits are active in many


def test_projective_forces_are_exactly_zero_inside_the_limits():
    pkg = _pkg()
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.linalg.det(Q))
    rows = []
    for sv in ([1.0, 1.0, 1.0], [1.2, 0.9, 0.95], [0.98, 1.05, 1.0], [1.3, 0.8, 1.0]):      # products 1, 1.026, 1.029, 1.04: inside [0.9, 1.1]
        rows.append((Q @ np.diag(sv) @ (np.eye(3) + 0.0)).T.reshape(9))
        rows.append((Q @ np.diag(sv) @ Q.T).T.reshape(9))
    g = pkg.gradient_query("TET_VOLUME", np.array(rows), PARAMS["TET_VOLUME"], None, SCALE)
    assert g.shape == (8, 9) and not g.any() and not np.signbit(g).any()
    out = pkg.gradient_query("TET_VOLUME", (Q @ np.diag([1.3, 1.0, 1.0])).T.reshape(1, 9), PARAMS["TET_VOLUME"], None, SCALE)
    assert np.abs(out).max() > 1e-3 * SCALE      # 1.3 > 1.1: active
    tri = []
    for sv in ([1.0, 1.0], [1.2, 0.85], [0.95, 1.1]):      # areas 1, 1.02, 1.045: inside [0.9, 1.1]
        tri.append((Q[:, :2] @ np.diag(sv)).T.reshape(6))
    g = pkg.gradient_query("TRI_AREA", np.array(tri), PARAMS["TRI_AREA"], None, SCALE)
    assert g.shape == (3, 6) and not g.any()
    out = pkg.gradient_query("TRI_AREA", (Q[:, :2] @ np.diag([1.3, 1.0])).T.reshape(1, 6), PARAMS["TRI_AREA"], None, SCALE)
    assert np.abs(out).max() > 1e-3 * SCALE


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. known answers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.5, 1.0, 1.2, 3.0])
def test_known_answers_uniform_scale(alpha):
    """d = alpha I: g is a multiple of I, the stress is hydrostatic and von Mises is 0.  The closed forms are evaluated in double by
    other operations than gradient.hpp's: 32 u relative to the sum of the absolute terms covers both sides' roundings (fewer than 16 each)"""
    pkg = _pkg()
    d = (alpha * np.eye(3)).reshape(1, 9)
    V = SCALE
    mu, lam = PARAMS["TET_NH"][:2]
    L = math.log(alpha ** 6)
    e = 0.5 * (alpha * alpha - 1.0)
    want = dict(TET_NH=(V * (mu * alpha + (0.5 * lam * L - mu) / alpha), V * (mu * alpha + (0.5 * lam * abs(L) + mu) / alpha)),
                TET_STVK=(V * alpha * (2 * mu * e + 3 * lam * e), V * alpha * (2 * mu + 3 * lam) * 0.5 * (alpha * alpha + 1.0)))
    for kind, (gs, gabs) in want.items():
        g = pkg.gradient_query(kind, d, PARAMS[kind], None, V).reshape(3, 3)
        assert g[0, 0] == g[1, 1] == g[2, 2] and not (g - np.diag(np.diag(g))).any(), (kind, g)
        assert abs(g[0, 0] - gs) <= 32 * U * gabs, (kind, g[0, 0], gs)
        st = pkg.stress_query(kind, d, PARAMS[kind], V)[0]
        p, pabs = gs * alpha / (V * alpha ** 3), gabs * alpha / (V * alpha ** 3)
        assert st[0] == st[1] == st[2] and not st[3:6].any() and st[6] == 0.0, (kind, st)
        assert abs(st[0] - p) <= 40 * U * pabs, (kind, st[0], p)
        if alpha == 1.0:
            assert g[0, 0] == 0.0 and st[0] == 0.0      # rest: no force, no stress


def test_known_answers_spring_stvk_uniaxial_and_symmetry():
    pkg = _pkg()
    k, L = PARAMS["SPRING"][0], SPRING_L
    r = np.zeros((1, 12)); r[0, 0] = L
    g = pkg.gradient_query("SPRING", [[2 * L, 0.0, 0.0]], PARAMS["SPRING"], r, k)
    assert g[0, 0] == k * L and g[0, 1] == 0.0 and g[0, 2] == 0.0      # twice the rest length: k (2 L - L), exact in double
    g = pkg.gradient_query("SPRING", [[0.0, 0.0, 0.0]], PARAMS["SPRING"], r, k)
    assert not g.any()      # |d| = 0: p = 0 (energy.hpp)
    # StVK under a uniaxial stretch d = diag(a, 1, 1): E = diag(e, 0, 0), S = diag((2 mu + lambda) e, lambda e, lambda e), g = s d S
    a = 1.25
    mu, lam = PARAMS["TET_STVK"][:2]
    e = 0.5 * (a * a - 1.0)
    d = np.diag([a, 1.0, 1.0]).reshape(1, 9)
    g = pkg.gradient_query("TET_STVK", d, PARAMS["TET_STVK"], None, SCALE).reshape(3, 3)
    want = SCALE * np.diag([a * (2 * mu + lam) * e, lam * e, lam * e])
    assert not (g - np.diag(np.diag(g))).any() and np.abs(g - want).max() <= 32 * U * SCALE * a * (2 * mu + lam) * 0.5 * (a * a + 1.0)
    st = pkg.stress_query("TET_STVK", d, PARAMS["TET_STVK"], SCALE)[0]
    sxx, syy = a * (2 * mu + lam) * e, lam * e / a      # sigma = g d^T / (V J), J = a
    assert abs(st[0] - sxx) <= 40 * U * abs(sxx) * (a * a + 1) / (a * a - 1) and abs(st[1] - syy) <= 40 * U * abs(syy) * (a * a + 1) / (a * a - 1) and st[1] == st[2]
    vm = abs(sxx - syy)
    assert not st[3:6].any() and abs(st[6] - vm) <= 48 * U * (abs(sxx) + abs(syy)) * (a * a + 1) / (a * a - 1)
    # symmetric by construction: for the exact kinds g d^T is symmetric up to rounding, and the six values are its symmetrised entries
    dd = exact_inputs("TET_NH")
    for kind in ("TET_NH", "TET_STVK"):
        g = pkg.gradient_query(kind, dd, PARAMS[kind], None, SCALE).reshape(-1, 3, 3).transpose(0, 2, 1)      # g[e][i][c]
        M = dd.reshape(-1, 3, 3).transpose(0, 2, 1)
        J = np.linalg.det(M)
        t = np.einsum("eic,ejc->eij", g, M) / (SCALE * J)[:, None, None]
        tabs = np.einsum("eic,ejc->eij", np.abs(g), np.abs(M)).max((1, 2)) / (SCALE * J)
        # |t_ij - t_ji|: g's own rounding (analytic_rounding, amplified by |d| / (V J)) and 8 u of the product's absolute terms
        amp = analytic_rounding(kind, dd, None) * np.abs(M).sum((1, 2)) / (SCALE * J)
        assert (np.abs(t - t.transpose(0, 2, 1)).max((1, 2)) <= 2 * amp + 8 * U * tabs).all(), kind
        st = pkg.stress_query(kind, dd, PARAMS[kind], SCALE)
        sym = 0.5 * (t + t.transpose(0, 2, 1))
        six = np.stack([sym[:, 0, 0], sym[:, 1, 1], sym[:, 2, 2], sym[:, 0, 1], sym[:, 0, 2], sym[:, 1, 2]], axis=1)
        assert (np.abs(st[:, :6] - six).max(1) <= 8 * U * tabs).all(), kind
        vm = np.sqrt(0.5 * ((six[:, 0] - six[:, 1]) ** 2 + (six[:, 1] - six[:, 2]) ** 2 + (six[:, 2] - six[:, 0]) ** 2) + 3 * (six[:, 3:] ** 2).sum(1))
        assert (np.abs(st[:, 6] - vm) <= 64 * U * tabs).all() and (st[:, 6] >= 0).all(), kind


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. argument checks, 5. a host-only context, 6. the C++ mirror compiles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_query_argument_checks():
    pkg = _pkg()
    L = pkg.lib()
    d = np.eye(3).reshape(1, 9).copy(); par = np.array([[1.0, 1.0, 5.0]]); rest = np.zeros((1, 12)); sc = np.ones(1)
    out = np.full(9, 7.0); st = np.full(7, 7.0)
    p = lambda a: a.ctypes.data_as(pkg._dp)      # noqa: E731
    gq, sq = L.admm_hip_gradient_query, L.admm_hip_stress_query
    assert gq(KIND["TET_NH"], 1, p(d), p(par), p(rest), p(sc), p(out)) == 0 and not out.any()      # rest: exactly zero
    assert sq(KIND["TET_NH"], 1, p(d), p(par), p(sc), p(st)) == 0 and not st.any()
    for kind in (-1, KIND["COLLISION"], 11, 99):      # not evaluated / unknown
        assert gq(kind, 1, p(d), p(par), p(rest), p(sc), p(out)) == 1, kind
    for kind in (-1, KIND["COLLISION"], KIND["BEND"], KIND["TRI_FUNG"], KIND["SPRING"], KIND["ANCHOR"], 11, 99):      # no tet kind
        assert sq(kind, 1, p(d), p(par), p(sc), p(st)) == 1, kind
    for hole in range(5):      # a NULL array with n > 0
        a = [p(d), p(par), p(rest), p(sc), p(out)]
        a[hole] = None
        assert gq(KIND["TET_NH"], 1, *a) == 1, hole
    for hole in range(4):
        a = [p(d), p(par), p(sc), p(st)]
        a[hole] = None
        assert sq(KIND["TET_NH"], 1, *a) == 1, hole
    assert gq(KIND["TET_NH"], 0, None, None, None, None, None) == 0 and sq(KIND["TET_NH"], 0, None, None, None, None) == 0
    assert gq(KIND["TET_NH"], -1, p(d), p(par), p(rest), p(sc), p(out)) == 1 and sq(KIND["TET_NH"], -1, p(d), p(par), p(sc), p(st)) == 1
    with pytest.raises(pkg.AdmmHipError):
        pkg.gradient_query(99, d, par, rest, sc)
    with pytest.raises(pkg.AdmmHipError):
        pkg.stress_query("BEND", d, [20.0], sc)
    assert pkg.gradient_query("SPRING", np.zeros((0, 3)), PARAMS["SPRING"], None, 1.0).shape == (0, 3)
    assert pkg.stress_query("TET_STVK", np.zeros((0, 9)), PARAMS["TET_STVK"], 1.0).shape == (0, 7)


def test_cpp_mirror_compiles_and_a_host_only_context_refuses(pkg):
    """the class mirror's force surface compiles without a GPU; a host-only context has no gradient path (no CPU fallback): the energy
    entries' error code"""
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_forces", pkg))
    X, tets = pkg.meshgen.bar(1, 1, 1, h=H)
    s = build_system(X, np.ones(3 * X.shape[0]), [("TET_NH", tets, PARAMS["TET_NH"])], device_id=-1)
    s.initialize()
    with pytest.raises(pkg.AdmmHipError, match="error 2"):
        s.energy()
    for call in (s.node_forces, lambda: s.batch_gradient(0), lambda: s.batch_stress(0), lambda: s.batch_gradient_dx(0, np.tile(np.eye(3).reshape(9), (6, 1)))):
        with pytest.raises(pkg.AdmmHipError, match="error 2"):
            call()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 130)      # a lone lane, a full wave, a one-lane tail, two full blocks and a tail


def sized_system(kind):
    """one context whose batches are all of `kind`, with 1, 63, 64, 65 and 130 elements -> (system, X, [idx per batch])"""
    mg = _pkg().meshgen
    if kind in TET_KINDS:
        X, elems = mg.bar(*BAR, h=H)
    elif kind == "ANCHOR":
        X, _ = mg.bar(5, 5, 10, h=H)
        elems = np.arange(X.shape[0], dtype=np.int32)[:, None]      # disjoint ranges: a node is held once
    else:
        X, tris, hinges, edges = cloth_mesh()
        elems = np.tile(tris if kind in TRI_KINDS else (hinges if kind == "BEND" else edges), (3, 1))
    assert elems.shape[0] >= (sum(SIZES) if kind == "ANCHOR" else max(SIZES))
    if kind == "ANCHOR":
        cuts = np.cumsum((0,) + SIZES)
        idx = [elems[cuts[i]:cuts[i + 1], 0] for i in range(len(SIZES))]
        _, tets = mg.bar(5, 5, 10, h=H)
        forces = [("TET_LINEAR", tets, PARAMS["TET_LINEAR"])] + [("ANCHOR", i, PARAMS["ANCHOR"]) for i in idx]
    else:
        idx = [elems[:n] for n in SIZES]
        forces = [(kind, i, PARAMS[kind]) for i in idx]
        if kind in TET_KINDS:      # Neo-Hookean twins on the same tets: their scale is the rest volume itself
            forces += [("TET_NH", i, PARAMS["TET_NH"]) for i in idx]
    s = build_system(X, np.ones(3 * X.shape[0]), forces)
    s.initialize()
    return s, X, idx, (1 if kind == "ANCHOR" else 0)


def kind_inputs(kind):
    if kind == "ANCHOR":
        return np.random.default_rng(5).standard_normal((200, 3))
    inp = inputs(kind)
    return np.roll(inp, inp.shape[0] - 4096, axis=0)      # the hand-made cases first: every batch of more than a few elements has its not-finite ones


@gpu
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_batch_gradient_dx_is_bitwise_gradient_query(pkg, kind):
    s, X, idxs, b0 = sized_system(kind)
    inp = kind_inputs(kind)
    any_bad = False
    x = deform(X)
    s.m_x = x.ravel()
    for k, n in enumerate(SIZES):
        b = b0 + k
        dx = np.ascontiguousarray(inp[:n] if n > 1 else inp[40:41])
        rest = s.read_rest(b)["rest"]
        if kind == "ANCHOR":
            rest = np.zeros((n, 12)); rest[:, :3] = X[idxs[k]]      # a static anchor's target: where it was added
        want = pkg.gradient_query(kind, dx, PARAMS[kind], rest, s.energy_scale(b))
        buf = np.full((n + 1, KIND_ROWS[KIND[kind]]), -12345.0)
        got = s.batch_gradient_dx(b, dx, out=buf[:n])
        assert np.all(buf[n:] == -12345.0), (kind, n, "wrote past g")
        assert _same_bits(got, want), (kind, n, np.nonzero(_bits(got) != _bits(want))[0][:8])
        any_bad |= bool(np.isnan(got).any())
        # the override is gone afterwards: the gathered gradient is that of the state
        g, cf, bad = s.batch_gradient(b)
        assert g.shape == want.shape and cf.shape == (n, KIND_NODES[KIND[kind]], 3) and bad == int(np.isnan(g).any(1).sum())
        if kind in TET_KINDS:      # the stress of the gathered rows, bitwise the host twin on D_i x rebuilt here
            rows = element_dx(kind, idxs[k], rest, x)
            assert _same_bits(g, pkg.gradient_query(kind, rows, PARAMS[kind], rest, s.energy_scale(b))), (kind, n)
            vol = s.energy_scale(len(SIZES) + k)
            st, nbad = s.batch_stress(b)
            want_st = pkg.stress_query(kind, rows, PARAMS[kind], vol)
            assert _same_bits(s.energy_scale(b), vol if kind in ("TET_NH", "TET_STVK") else PARAMS[kind][0] * vol), (kind, n, "the rest volume differs from the library's")
            assert st.shape == (n, 7) and _same_bits(st, want_st), (kind, n, np.nonzero(_bits(st) != _bits(want_st))[0][:8])
            assert nbad == int(np.isnan(st).any(1).sum())
    assert any_bad == (kind in ("TET_NH", "TRI_FUNG"))


def free_node_scene():
    """element_cases.mixed_forces() -- tets of four kinds, cloth triangles of three, hinges, springs, anchors, a collision batch -- and one
    more node that no elastic element touches (the collision batch, which is not evaluated, covers it too)"""
    X, M3, forces = mixed_forces(PARAMS)
    X = np.concatenate([X, [[0.9, 0.4, 0.2]]]); M3 = np.concatenate([M3, [0.01] * 3])
    forces = [(k, (np.arange(X.shape[0], dtype=np.int32) if k == "COLLISION" else i), p) for k, i, p in forces]
    return X, M3, forces


def expected_gradient(s, b, kind, idx, x, X0):
    """-> (g, corner forces) of the batch's local elements from the host twin on D_i x rebuilt here, -D_i^T g in the documented order"""
    pkg = _pkg()
    loc = s.local_elements(b)
    idx = np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]])[loc]
    rest = s.read_rest(b)["rest"][loc]
    scale = s.energy_scale(b)
    n = idx.shape[0]
    if kind == "ANCHOR":
        r = np.zeros((n, 12)); r[:, :3] = X0[idx[:, 0]]
        g = pkg.gradient_query("ANCHOR", x.reshape(-1, 3)[idx[:, 0]], PARAMS["ANCHOR"], r, scale)
    else:
        g = pkg.gradient_query(kind, element_dx(kind, idx, rest, x), PARAMS[kind], rest, scale)
    cf = np.zeros((n, idx.shape[1], 3))
    if kind in TET_KINDS:
        for c in range(4):
            for j in range(3):
                cf[:, c, j] = -((g[:, j] * rest[:, c] + g[:, 3 + j] * rest[:, c + 4]) + g[:, 6 + j] * rest[:, c + 8])
    elif kind in TRI_KINDS:
        for c in range(3):
            for j in range(3):
                cf[:, c, j] = -(g[:, j] * rest[:, c] + g[:, 3 + j] * rest[:, c + 3])
    elif kind == "BEND":      # rows x0 - x2, x3 - x2, x1 - x2
        cf[:, 0] = -g[:, 0:3]; cf[:, 1] = -g[:, 6:9]; cf[:, 3] = -g[:, 3:6]; cf[:, 2] = (g[:, 0:3] + g[:, 3:6]) + g[:, 6:9]
    elif kind == "SPRING":
        cf[:, 0] = -g; cf[:, 1] = g
    else:
        cf[:, 0] = -g
    cf[np.isnan(g).any(1)] = 0.0      # an element whose g is not finite adds nothing
    return g, cf, idx


def expected_node_forces(s, forces, x, X0):
    """the sequential sums in the documented CSR order -- batch, local element, the element's corners as listed -- by the documented
    compensated rule (kernels_gradient.hpp): s = c = 0; per term v: t = s + v, bp = t - s, e = (s - (t - bp)) + (v - bp), s = t, c = c + e;
    the result is s + c.  numpy's float64 rounds every operation as the device does."""
    nn = X0.shape[0]
    S, Cc = np.zeros((2, nn, 3)), np.zeros((2, nn, 3))
    bad = skipped = 0
    for b, (kind, idx, _) in enumerate(forces):
        if kind == "COLLISION":
            skipped += 1
            continue
        g, cf, lidx = expected_gradient(s, b, kind, idx, x, X0)
        bad += int(np.isnan(g).any(1).sum())
        w = 1 if kind == "ANCHOR" else 0
        for el in range(lidx.shape[0]):
            for c in range(lidx.shape[1]):
                i = lidx[el, c]
                v, s0 = cf[el, c], S[w, i].copy()
                t = s0 + v
                bp = t - s0
                e = (s0 - (t - bp)) + (v - bp)
                S[w, i] = t; Cc[w, i] = Cc[w, i] + e
    fe, fa = S[0] + Cc[0], S[1] + Cc[1]
    return fe, fa, bad, skipped


@pytest.fixture(scope="module")
def scene(pkg):
    X, M3, forces = free_node_scene()
    s = build_system(X, M3, forces)
    s.initialize()
    x = deform(X, fold=True)
    s.m_x = x.ravel()
    return dict(s=s, X=X, M3=M3, forces=forces, x=x)


@gpu
def test_gather_path_corner_forces_and_node_sums_are_bitwise(pkg, scene, monkeypatch):
    s, forces, x, X = scene["s"], scene["forces"], scene["x"], scene["X"]
    kinds = set()
    for b, (kind, idx, _) in enumerate(forces):
        g, cf, bad = s.batch_gradient(b)
        if kind == "COLLISION":
            assert g.shape == (X.shape[0], 3) and not g.any() and not cf.any() and bad == 0
            continue
        wg, wcf, _ = expected_gradient(s, b, kind, idx, x, X)
        assert _same_bits(g, wg), (b, kind, np.nonzero(_bits(g) != _bits(wg))[0][:8])
        assert _same_bits(cf, wcf), (b, kind, np.nonzero(_bits(cf) != _bits(wcf))[0][:8])
        assert bad == int(np.isnan(wg).any(1).sum())
        kinds.add(kind)
    assert kinds == set(ALL_KINDS)
    assert s.batch_gradient(0)[2] > 0      # the fold inverts Neo-Hookean tets of the first batch
    fe, fa, bad, skipped = expected_node_forces(s, forces, x, X)
    nf = s.node_forces()
    assert _same_bits(nf["elastic"], fe), np.nonzero(_bits(nf["elastic"]) != _bits(fe))[0][:8]
    assert _same_bits(nf["anchor"], fa)
    assert nf["n_nonfinite"] == bad > 0 and nf["batches_skipped"] == skipped == 1
    free = X.shape[0] - 1
    assert not nf["elastic"][free].any() and not nf["anchor"][free].any() and not np.signbit(nf["elastic"][free]).any()
    assert np.abs(nf["elastic"]).max() > 0.0 and np.abs(nf["anchor"]).max() > 0.0 and np.isfinite(nf["elastic"]).all()
    assert (np.abs(nf["anchor"]).sum(1) > 0).sum() <= forces[9][1].size      # only held nodes carry an anchor force
    again = s.node_forces()
    assert _same_bits(again["elastic"], nf["elastic"]) and _same_bits(again["anchor"], nf["anchor"])
    # a context created under other launch knobs returns the same bits
    monkeypatch.setenv("ADMM_HIP_TPB", "16"); monkeypatch.setenv("ADMM_HIP_LOCAL_MULTI", "0"); monkeypatch.setenv("ADMM_HIP_PRERED", "0")
    t = build_system(X, scene["M3"], forces)
    t.initialize()
    t.m_x = x.ravel()
    nt = t.node_forces()
    assert _same_bits(nt["elastic"], nf["elastic"]) and _same_bits(nt["anchor"], nf["anchor"]) and nt["n_nonfinite"] == bad
    for b in range(len(forces)):
        for a, c in zip(s.batch_gradient(b)[:2], t.batch_gradient(b)[:2]):
            assert _same_bits(a, c), b


def check_forces_against_energy_differences(s, forces, X0, x, edge):
    """f_elastic + f_anchor = -d(elastic + anchor)/dx by central differences over every coordinate, with the bound the issue sets,
        |f + FD_h| <= |FD_h - FD_2h| + 2^-53 |E_total| / h
    (truncation: FD_h = -f + c h^2 + O(h^4), so FD_2h - FD_h = 3 c h^2 + O(h^4) bounds it three times over; E_total: the largest
    |elastic + anchor| of the evaluations).  h = 2^-12, half a percent of an edge.  The energies are double, and their true rounding
    in a difference is 2^-53 of the ABSOLUTE terms of the elements at the node -- tens of times |E_total|, since I1 - 3 cancels near
    rest -- so the stated rounding term alone is too small at any h; at h = 2^-12 the truncation estimate exceeds that rounding by
    seven orders of magnitude (E3 h^2 with the third derivative E3 ~ s mu / edge^3, against 1e-15 / h), and two thirds of it are
    spare.  The bound is second order in h / edge: asserted to stay below (h / edge) of the largest force, so that a wrong
    coefficient cannot meet it."""
    h = 2.0 ** -12
    s.m_x = x.ravel()
    nf = s.node_forces()
    f = nf["elastic"] + nf["anchor"]
    assert nf["n_nonfinite"] == 0
    emax = [0.0]

    def total(xx):
        s.m_x = xx.ravel()
        e = s.energy()
        assert e["n_infinite"] == 0
        emax[0] = max(emax[0], abs(e["elastic"] + e["anchor"]))
        return e["elastic"] + e["anchor"]
    fds = np.zeros((2,) + x.shape)
    for node in range(x.shape[0]):
        for j in range(3):
            for k, hh in enumerate((h, 2 * h)):
                xp, xm = x.copy(), x.copy()
                xp[node, j] += hh; xm[node, j] -= hh
                fds[k, node, j] = (total(xp) - total(xm)) / (2 * hh)
    s.m_x = x.ravel()
    bound = np.abs(fds[0] - fds[1]) + U * emax[0] / h
    err = np.abs(f + fds[0])
    fmax = np.abs(f).max()
    print("forces against energy differences: largest error / bound %.3g; largest bound / largest |f| %.3g (h / edge %.3g); largest |f| %.3g; |E_total| %.3g"
          % ((err / bound).max(), bound.max() / fmax, h / edge, fmax, emax[0]))
    assert (err <= bound).all(), (np.unravel_index((err / bound).argmax(), err.shape), (err / bound).max())
    assert bound.max() <= (h / edge) * fmax
    return nf


@gpu
def test_forces_are_minus_the_energy_differences_bar(pkg):
    """also: the elastic forces of the anchor-free bar sum to zero and have no net torque.  A tet's corner forces are -g B(c, .) with
    sum_c B(c, r) = 0 up to the rounding of B, whatever g is, so the sum over all nodes is rounding alone: the 3 products and 2 sums of
    a corner force, the rounding of B and the sequential node sums and the final sum of n values, each relative to a partial sum of at
    most sum |corner forces|: 8 n u sum |corner forces|, n = the node count (sum |f| of the issue taken over the corner forces the node
    sums are made of: the node sums themselves cancel).  Torque: sum_c x_c x f_c is the axial vector of d g^T - g d^T, zero because
    g d^T = s (mu d d^T + q J I) is symmetric; in double g errs by a few u of its absolute terms s (mu |d| + |q| |cof|), about 1 / strain
    times |g|, which the factor n covers at this deformation (strain 0.1, n = 36): 8 n u sum (|x| x |corner forces|)."""
    mg = pkg.meshgen
    X, tets = mg.bar(2, 2, 3, h=H)
    assert X.shape[0] == 36
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    forces = [("TET_NH", tets, PARAMS["TET_NH"]), ("ANCHOR", mg.bar_anchor_nodes(2, 2), PARAMS["ANCHOR"])]
    s = build_system(X, m3, forces)
    s.initialize()
    x = deform(X, amp=0.08)
    check_forces_against_energy_differences(s, forces, X, x, H)
    free = build_system(X, m3, forces[:1])
    free.initialize()
    free.m_x = x.ravel()
    nf = free.node_forces()
    fe = nf["elastic"]
    assert not nf["anchor"].any() and nf["n_nonfinite"] == 0
    _, cf, _ = free.batch_gradient(0)
    n = X.shape[0]
    acf = np.abs(cf).sum()
    net = fe.sum(0)
    xc = x[tets]      # [e][c][3]
    torque = np.cross(x, fe).sum(0)
    atq = (np.abs(xc)[:, :, [1, 2, 0]] * np.abs(cf)[:, :, [2, 0, 1]] + np.abs(xc)[:, :, [2, 0, 1]] * np.abs(cf)[:, :, [1, 2, 0]]).sum()
    print("balance: |net force| %.3g (bound %.3g), |net torque| %.3g (bound %.3g), largest |f| %.3g" % (np.abs(net).max(), 8 * n * U * acf, np.abs(torque).max(), 8 * n * U * atq, np.abs(fe).max()))
    assert np.abs(fe).max() > 1.0
    assert np.abs(net).max() <= 8 * n * U * acf
    assert np.abs(torque).max() <= 8 * n * U * atq


@gpu
def test_forces_are_minus_the_energy_differences_cloth(pkg):
    mg = pkg.meshgen
    X, tris = mg.sym_plane(3, 3)
    hinges = mg.bend_hinges(tris)
    e = np.sort(np.vstack([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    edges = np.unique(e, axis=0).astype(np.int32)
    X = 0.3 * X
    m3 = np.full(3 * X.shape[0], 0.5 / X.shape[0])
    half = tris.shape[0] // 2
    forces = [("TRI_STRAIN", tris[:half], PARAMS["TRI_STRAIN"]), ("TRI_FUNG", tris[half:], PARAMS["TRI_FUNG"]), ("BEND", hinges, PARAMS["BEND"]),
              ("SPRING", edges, PARAMS["SPRING"]), ("ANCHOR", np.array([0, 3], dtype=np.int32), PARAMS["ANCHOR"])]
    s = build_system(X, m3, forces)
    s.initialize()
    k = np.arange(X.size, dtype=np.float64).reshape(X.shape)
    x = X * (1.0 + 0.05 * np.sin(1.7 * k)) + 0.02 * np.cos(0.9 * k)      # stretched, sheared and bent out of its plane
    check_forces_against_energy_differences(s, forces, X, x, float(np.linalg.norm(X[edges[:, 0]] - X[edges[:, 1]], axis=1).min()))


def call_everything(s, forces):
    nf = s.node_forces()
    assert np.isfinite(nf["elastic"]).all() and np.abs(nf["elastic"]).max() > 0.0 and nf["n_nonfinite"] == 0
    for b, (kind, _, _) in enumerate(forces):
        s.batch_gradient(b)
        if kind in TET_KINDS:
            s.batch_stress(b)
        if kind != "COLLISION":
            n = s.local_elements(b).size
            s.batch_gradient_dx(b, np.tile((np.eye(3).reshape(9) if KIND_ROWS[KIND[kind]] == 9 else np.eye(3).reshape(9)[:KIND_ROWS[KIND[kind]]]), (n, 1)))


@gpu
def test_no_side_effects(pkg):
    """modelled on test_energy.test_no_side_effects.  Ten graph-replayed frames of free_node_scene() without its Fung triangles, with and
    without the calls between the frames: x, v, every batch's u, warm starts and iteration counts keep their bits, and so do the captured
    graphs and their launch count.  The Fung triangles are left out of the ten frames because with them the scene's x is NaN from its
    ninth frame on (from its first at test_energy's deformation), and a NaN state shows nothing; they take part in the second half: the
    whole scene, one frame, u, z and the warm starts read before and after the calls, and the next frame against a twin that made no call."""
    X, M3, forces_all = free_node_scene()
    forces = [f for f in forces_all if f[0] != "TRI_FUNG"]
    x0 = deform(X, amp=0.002)
    runs = {}
    for mode in ("plain", "forces"):
        s = build_system(X, M3, forces)
        s.initialize()
        s.m_x = x0.ravel()
        for f in range(10):
            s.step(4)
            if mode == "forces" and f % 2 == 1:      # between frames of a graph-replayed context
                call_everything(s, forces)
        runs[mode] = (_state(s, forces), s.graph_state())
    assert all(np.isfinite(a).all() for a in runs["plain"][0])
    for a, b in zip(runs["plain"][0], runs["forces"][0]):
        assert _same_bits(a, b)
    gp, gf = runs["plain"][1], runs["forces"][1]
    assert gp == gf, (gp, gf)      # the same graphs and the same number of launches: no call dropped one
    assert gp["iter_graph"] and gp["frame_graph_iters"] == 4 and gp["graph_launches"] >= 9, gp      # the frame graph of four iterations, kept and launched
    twins = []
    for mode in ("plain", "forces"):
        s = build_system(X, M3, forces_all)
        s.initialize()
        s.m_x = x0.ravel()
        s.step(4)
        if mode == "forces":
            before = [s.read_local(b) for b in range(len(forces_all))]
            call_everything(s, forces_all)
            for b, old in enumerate(before):
                new = s.read_local(b)
                for key in old:      # u, z, the warm starts, the iteration counts
                    assert _same_bits(np.asarray(old[key], dtype=np.float64), np.asarray(new[key], dtype=np.float64)), (b, key)
        s.step(4)
        twins.append(_state(s, forces_all) + [s.graph_state()])
    assert all(np.isfinite(a).all() for a in twins[0][:2])
    for a, b in zip(twins[0][:-1], twins[1][:-1]):
        assert _same_bits(a, b)
    assert twins[0][-1] == twins[1][-1]


@gpu
def test_shards(pkg, monkeypatch):
    """the ranks' vectors add up to the one-rank vector within 2^-52 sum_r |share_r| per component, share_r the vector rank r returns (the
    bound the issue sets).  The gather's compensated sum makes every share and the one-rank value the exact sum of its corner forces
    rounded once (to second order): with S = S_0 + S_1 exact, |s_0 + s_1 - s| <= 2^-53 (|S_0| + |S_1| + |S|) <= 2^-52 sum |share|.  The
    ranks' vectors are added exactly here (math.fsum rounds the exact sum of s_0, s_1 and -s once), since a rounded addition would spend
    another 2^-53 |S| of the bound.  A node whose elements all live on one rank gets that rank's vector bit for bit."""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    mg = pkg.meshgen
    dims = (3, 3, 12)
    X, tets = mg.bar(*dims, h=H)
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    forces = [("TET_NH", tets[:300], PARAMS["TET_NH"]), ("TET_STVK", tets[300:], PARAMS["TET_STVK"]), ("ANCHOR", mg.bar_anchor_nodes(dims[0], dims[1]), PARAMS["ANCHOR"])]
    one = build_system(X, m3, forces)
    one.initialize()
    world = 2
    shards = [build_system(X, m3, forces, rank=r, world=world) for r in range(world)]
    for sh, hk in zip(shards, _thread_allreduce_hooks(world)):
        sh.set_shard_mode("subtree"); sh.set_allreduce(hk)
    pkg.initialize_together(shards)
    x = deform(X)
    for s in [one] + shards:
        s.m_x = x.ravel()
    f1 = one.node_forces()
    fs = [s.node_forces() for s in shards]
    for b, (kind, idx, _) in enumerate(forces):
        g1, cf1, _ = one.batch_gradient(b)
        seen = np.zeros(g1.shape[0], dtype=int)
        for s in shards:
            loc = s.local_elements(b)
            g, cf, _ = s.batch_gradient(b)
            assert g.shape[0] == loc.size and _same_bits(g, g1[loc]) and _same_bits(cf, cf1[loc]), (b, kind)      # the local elements only
            if kind in TET_KINDS:
                assert _same_bits(s.batch_stress(b)[0], one.batch_stress(b)[0][loc])
            seen[loc] += 1
        assert (seen == 1).all()
    assert min(s.local_elements(0).size + s.local_elements(1).size for s in shards) > 0
    assert min(s.local_elements(b).size for s in shards for b in (0, 2)) == 0      # a tet and the anchor batch are empty on one rank
    for key in ("elastic", "anchor"):
        share = sum(np.abs(f[key]) for f in fs)
        diff = np.array([[abs(math.fsum([f[key][i, j] for f in fs] + [-f1[key][i, j]])) for j in range(3)] for i in range(X.shape[0])])
        print("shards, %s: largest |sum of the ranks - one rank| / (2^-52 sum |share|) %.3g; components that differ: %d of %d with two shares"
              % (key, (diff / np.maximum(2.0 ** -52 * share, 1e-300)).max(), int((diff > 0).sum()), int((np.minimum(*[np.abs(f[key]) for f in fs]) > 0).sum())))
        assert (diff <= 2.0 ** -52 * share).all(), key
        assert max(np.abs(f[key]).max() for f in fs) > 0.0
    assert sum(f["n_nonfinite"] for f in fs) == f1["n_nonfinite"] == 0


@gpu
def test_one_inverted_tet_in_a_batch_of_65(pkg):
    mg = pkg.meshgen
    X, tets = mg.bar(*BAR, h=H)
    node = int(tets[0][0])      # 65 tets of which only the first holds `node`; its other corners have further tets
    tets = np.vstack([tets[:1]] + [t[None] for t in tets[1:] if node not in t][:64])
    assert tets.shape[0] == 65
    count = np.bincount(tets.ravel(), minlength=X.shape[0])
    e = 0
    others = [c for c in tets[e] if c != node]
    x = deform(X)
    a, b, c = x[others]
    nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm)
    x[node] = x[node] - 2.0 * np.dot(x[node] - a, nrm) * nrm      # reflected through the opposite face: that one tet is inverted
    forces = [("TET_NH", tets, PARAMS["TET_NH"])]
    s = build_system(X, np.ones(3 * X.shape[0]), forces)
    s.initialize()
    s.m_x = x.ravel()
    g, cf, bad = s.batch_gradient(0)
    assert bad == 1 and np.isnan(g[e]).all() and np.isfinite(np.delete(g, e, axis=0)).all()
    assert not cf[e].any() and np.isfinite(cf).all()
    st, sbad = s.batch_stress(0)
    assert sbad == 1 and np.isnan(st[e]).all() and np.isfinite(np.delete(st, e, axis=0)).all()
    tot, per, ninf = s.batch_energy(0)
    assert ninf == 1 and np.isinf(per[e])
    nf = s.node_forces()
    assert nf["n_nonfinite"] == 1 and np.isfinite(nf["elastic"]).all()
    fe, _, _, _ = expected_node_forces(s, forces, x, X)      # (its corner forces are zeros there: the finite neighbours' shares only)
    assert _same_bits(nf["elastic"], fe)
    assert not nf["elastic"][node].any()      # its only tet is the inverted one
    for c in others:
        assert count[c] > 1 and nf["elastic"][c].any()


@gpu
def test_cpp_mirror(pkg, tmp_path):
    from test_cpp_host import compile_cpp
    mg = pkg.meshgen
    X, tets = mg.bar(*BAR, h=H)
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    anchors = mg.bar_anchor_nodes(BAR[0], BAR[1]).astype(np.int32)
    frames, iters = 2, 5
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        np.array([X.shape[0], tets.shape[0], anchors.size, 0], dtype=np.int32).tofile(f)
        X.ravel().tofile(f); m3.tofile(f); tets.astype(np.int32).tofile(f); anchors.tofile(f)
    r = subprocess.run([compile_cpp("scene_forces", pkg), str(inp), str(frames), str(iters)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    s = build_system(X, m3, [("TET_NH", tets, [1e5, 1e5, 5]), ("ANCHOR", anchors, PARAMS["ANCHOR"])])
    s.initialize()
    for _ in range(frames):
        s.step(iters)
    nf = s.node_forces()
    n3 = 3 * X.shape[0]
    assert lines[0] == "forces %d %d %d" % (n3, nf["n_nonfinite"], nf["batches_skipped"])
    got = np.array([[float.fromhex(v) for v in l.split()[1:3]] for l in lines[1:1 + n3]])
    assert _same_bits(got[:, 0], nf["elastic"].ravel()) and _same_bits(got[:, 1], nf["anchor"].ravel())
    st, _ = s.batch_stress(0)
    assert lines[1 + n3] == "stress %d" % st.size
    assert _same_bits([float.fromhex(l.split()[1]) for l in lines[2 + n3:2 + n3 + st.size]], st.ravel())
