"""Energies and the per-iteration ADMM objective (admm_hip_energy & co.; csrc/energy.hpp, csrc/kernels_energy.hpp).

CPU, through energy_query (the host evaluation of energy.hpp, the device's bits):
  1. the host twin against a restatement in np.longdouble written here from the table in include/admm_hip.h, the blended kinds'
     projections included (through the singular values: |d - U diag(n) V^T|^2 = sum (sigma_i - n_i)^2, sigma from a one-sided Jacobi
     in long double);
  2. known answers for a uniformly scaled bar and a uniformly scaled cloth;
  3. argument checks.
GPU: the kernels are bitwise energy_query on supplied rows (4) and on gathered rows (5), the sums (6), free fall (7), the per-iteration
objective history against fresh contexts (8), no side effects (9), shards (10), the C++ mirror (11).

The constants C of test 1 (|dE| <= C eps mag) are 4 x the host twin's largest observed ratio on the test's own inputs, rounded up to
a power of two; the observed maxima stand beside them (C_BOUND).
"""
import math
import os
import subprocess
import threading

import numpy as np
import pytest

from checkers import KIND, KIND_NODES, KIND_ROWS
from element_cases import (BAR, BEND_ALPHA, DT, EVALUATED, G, H, LD, SCALE, SPRING_L, TET_KINDS, TRI_KINDS, _bits, _pkg, _same_bits,
                           _state, build_system, cloth_mesh, deform, element_dx, inputs, ld_det3, ld_singular_values, mixed_forces, needs_ld)

gpu = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = dict(TET_NH=[1e5, 2e5, 5], TET_STVK=[1e5, 2e5, 5], TET_LINEAR=[4000.0], TET_VOLUME=[4000.0, 0.9, 1.1], TRI_FUNG=[50.0, 0.0, 0.0],
              TRI_STRAIN=[100.0, 0.95, 1.05, 1.0], TRI_AREA=[100.0, 3.0, 0.9, 1.1], SPRING=[300.0], BEND=[20.0])

# test 1: C and, beside it, the host twin's largest observed |dE| / (eps mag) against the long-double restatement on the inputs below
# (4096 random elements, seed 0, plus the hand-made cases).  TET_NH_LOW: the elements with 0 < J < 0.05, whose bound carries 1 / J.
C_BOUND = dict(TET_NH=(8, 1.82), TET_NH_LOW=(1, 0.188), TET_STVK=(2 ** 20, 2.42e5), TET_STVK_ABS=(2, 0.448), TET_LINEAR=(16, 3.46),
               TET_VOLUME=(32, 4.95), TRI_FUNG=(128, 24.5), TRI_STRAIN=(32, 5.11), TRI_AREA=(32, 4.17), SPRING=(4, 0.608), BEND=(4, 0.939))
# TET_STVK's ratio of 2.4e5 is no loss of accuracy: the magnitude the comparison is set against, s |d|^2_F, leaves out the material
# constants (mu = 1e5, lambda = 2e5 here) and the energy's quartic growth, E ~ s mu |d|^4 / 4.  Against the sum of the absolute terms,
# s [mu |(|d|^T |d| + I) / 2|^2_F + lambda / 2 tr^2((|d|^T |d| + I) / 2)], the largest ratio is 0.448; the test asserts both
# (TET_STVK_ABS is the one that would catch a wrong digit).  TRI_FUNG's 24.5: mag = s (|d|^2_F + mu / 2 (ex (1 + I1 + 3) + 1)) with ex =
# exp(I1 - 3), the exponential amplifying the absolute error of its argument; what is left is the cancellation in g = a b - c^2 that
# 1 / g then carries into I1 (the element with the largest ratio has a b / g = 19).


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (element_cases.inputs) and their rest data
# ---------------------------------------------------------------------------------------------------------------------------------
def rest_rows(kind, n):
    rest = np.zeros((n, 12))
    if kind == "SPRING":
        rest[:, 0] = SPRING_L
    if kind == "BEND":
        rest[:, :4] = BEND_ALPHA
    return rest


def host_energy(kind, d):
    return _pkg().energy_query(kind, d, PARAMS[kind], rest_rows(kind, d.shape[0]), SCALE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the long-double restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def ld_energy(kind, d):
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


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the host twin against the long-double restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _ratios(kind):
    d = inputs(kind)
    E = host_energy(kind, d)
    R, mag = ld_energy(kind, d)
    inf_h, inf_r = ~np.isfinite(E), ~np.isfinite(R.astype(np.float64))
    fin = ~inf_h & ~inf_r
    ratio = np.zeros(d.shape[0])
    ratio[fin] = (np.abs(E[fin].astype(LD) - R[fin]) / (LD(EPS) * mag[fin])).astype(np.float64)
    return d, E, inf_h, inf_r, ratio


@needs_ld
@pytest.mark.parametrize("kind", EVALUATED)
def test_host_twin_against_long_double(kind):
    d, E, inf_h, inf_r, ratio = _ratios(kind)
    assert np.array_equal(inf_h, inf_r), "the host twin and the restatement disagree on which elements are infinite: %s" % np.nonzero(inf_h != inf_r)[0]
    assert not np.isnan(E).any() and (E[~inf_h] >= 0.0).all() if kind != "TET_NH" else not np.isnan(E).any()
    rnd = slice(0, 4096)
    if kind in ("TET_NH", "TRI_FUNG"):
        frac = inf_h[rnd].mean()
        print("%s: %d infinite elements, %.2f %% of the random set" % (kind, inf_h.sum(), 100 * frac))
        assert inf_h.sum() >= 1 and frac <= 0.02
    else:
        assert not inf_h.any()
    if kind == "TET_NH":
        M = d.reshape(-1, 3, 3).transpose(0, 2, 1)
        J = np.linalg.det(M)
        fin = ~inf_h
        hi, lo = fin & (J >= 0.05), fin & (J < 0.05)
        print("TET_NH: J >= 0.05: %.2f %% of the random set, largest ratio %.3g;  0 < J < 0.05: %d elements, largest ratio x J %.3g"
              % (100 * hi[rnd].mean(), ratio[hi].max(), lo.sum(), (ratio[lo] * J[lo]).max() if lo.any() else 0.0))
        assert hi[rnd].mean() >= 0.98
        assert (ratio[hi] <= C_BOUND["TET_NH"][0]).all(), ratio[hi].max()
        assert (ratio[lo] * J[lo] <= C_BOUND["TET_NH_LOW"][0]).all(), (ratio[lo] * J[lo]).max()
        return
    print("%s: largest ratio %.3g" % (kind, ratio.max()))
    assert (ratio <= C_BOUND[kind][0]).all(), (ratio.max(), int(ratio.argmax()))
    if kind == "TET_STVK":
        R, _ = ld_energy(kind, d)
        _, mag = ld_energy("TET_STVK_ABS", d)
        r2 = (np.abs(E.astype(LD) - R) / (LD(EPS) * mag)).astype(np.float64)
        print("TET_STVK against the sum of its absolute terms: largest ratio %.3g" % r2.max())
        assert (r2 <= C_BOUND["TET_STVK_ABS"][0]).all(), r2.max()


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes (element_cases) and what the device is expected to give on them
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 270)      # a lone lane, a full wave, a one-lane tail, several blocks with a partial last one


def params_rows(kind, n):
    return np.tile(np.asarray(PARAMS[kind], dtype=np.float64), (n, 1))


def expected_batch_energy(s, b, kind, idx, x, host=None):
    """energy_query on the batch's local elements, fed with D_i x reproduced here"""
    pkg = _pkg()
    loc = s.local_elements(b)
    idx = np.asarray(idx).reshape(-1, KIND_NODES[KIND[kind]])[loc]
    rest = s.read_rest(b)["rest"][loc]
    scale = s.energy_scale(b)
    if kind == "ANCHOR":
        X0 = host
        r = np.zeros((idx.shape[0], 12)); r[:, :3] = X0[idx[:, 0]]
        return pkg.energy_query("ANCHOR", x.reshape(-1, 3)[idx[:, 0]], [-1.0, 1.0], r, scale)
    return pkg.energy_query(kind, element_dx(kind, idx, rest, x), PARAMS[kind], rest, scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. known answers (CPU: a host-only context supplies the rest data)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.5, 1.2, 3.0])
def test_known_answers_uniform_scale(scale):
    pkg = _pkg()
    mg = pkg.meshgen
    xb, tets = mg.bar(*BAR, h=H)
    xc, tris, hinges, edges = cloth_mesh()
    off = xb.shape[0]
    X = np.concatenate([xb, xc + np.array([1.0, 0.0, 0.0])])
    M3 = np.ones(3 * X.shape[0])
    forces = [("TET_NH", tets, PARAMS["TET_NH"]), ("TET_STVK", tets, PARAMS["TET_STVK"]), ("TET_LINEAR", tets, PARAMS["TET_LINEAR"]),
              ("SPRING", edges + off, PARAMS["SPRING"]), ("BEND", hinges + off, PARAMS["BEND"])]
    s = build_system(X, M3, forces, device_id=-1)
    s.initialize()
    x = scale * X
    V = BAR[0] * BAR[1] * BAR[2] * H ** 3
    sc = scale
    mu, lam = PARAMS["TET_NH"][:2]
    L = math.log(sc ** 6)
    e2 = 0.5 * (sc * sc - 1.0)
    k = PARAMS["TET_LINEAR"][0]
    Ls = np.linalg.norm(X[edges[:, 0] + off] - X[edges[:, 1] + off], axis=1)
    want = dict(TET_NH=V * (mu / 2 * (3 * sc * sc - L - 3) + lam / 8 * L * L), TET_STVK=V * (mu * 3 * e2 * e2 + lam / 2 * (3 * e2) ** 2),
                TET_LINEAR=V * k / 2 * 3 * (sc - 1.0) ** 2, SPRING=PARAMS["SPRING"][0] / 2 * (sc - 1.0) ** 2 * math.fsum(Ls * Ls), BEND=0.0)
    for b, (kind, idx, _) in enumerate(forces):
        E = expected_batch_energy(s, b, kind, idx, x)
        tot = math.fsum(E)
        if kind == "BEND":      # a flat sheet scaled uniformly stays flat: zero, against the size of the rows
            ref = PARAMS["BEND"][0] * (scale * scale) * float((element_dx(kind, idx, None, X) ** 2).sum())
            assert abs(tot) <= 1e-10 * ref, (kind, tot, ref)
            continue
        print("%s at scale %g: total %.17g, closed form %.17g, relative difference %.2e" % (kind, scale, tot, want[kind], abs(tot - want[kind]) / abs(want[kind])))
        assert abs(tot - want[kind]) <= 1e-10 * abs(want[kind]), (kind, tot, want[kind])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. argument checks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_energy_query_argument_checks():
    pkg = _pkg()
    L = pkg.lib()
    d = np.eye(3).reshape(1, 9).copy(); par = np.array([[1.0, 1.0, 5.0]]); rest = np.zeros((1, 12)); sc = np.ones(1); out = np.full(1, 7.0)
    p = lambda a: a.ctypes.data_as(pkg._dp)      # noqa: E731
    ok = lambda kind, n, *a: L.admm_hip_energy_query(kind, n, *a)      # noqa: E731
    assert ok(KIND["TET_NH"], 1, p(d), p(par), p(rest), p(sc), p(out)) == 0 and out[0] == 0.0      # rest: exactly zero
    for kind in (-1, KIND["COLLISION"], 11, 99):      # not evaluated / unknown
        assert ok(kind, 1, p(d), p(par), p(rest), p(sc), p(out)) == 1, kind
    for hole in range(5):      # a NULL array with n > 0
        a = [p(d), p(par), p(rest), p(sc), p(out)]
        a[hole] = None
        assert ok(KIND["TET_NH"], 1, *a) == 1, hole
    assert ok(KIND["TET_NH"], 0, None, None, None, None, None) == 0
    assert ok(KIND["TET_NH"], -1, p(d), p(par), p(rest), p(sc), p(out)) == 1
    with pytest.raises(pkg.AdmmHipError):
        pkg.energy_query(99, d, par, rest, sc)
    assert pkg.energy_query("SPRING", np.zeros((0, 3)), PARAMS["SPRING"], None, 1.0).shape == (0,)


def test_cpp_mirror_compiles_and_a_host_only_context_refuses(pkg):
    """the class mirror's energy surface compiles without a GPU; a host-only context has no energy path (no CPU fallback)"""
    from test_cpp_host import compile_cpp
    assert os.path.exists(compile_cpp("scene_energy", pkg))
    mg = pkg.meshgen
    X, tets = mg.bar(1, 1, 1, h=H)
    s = build_system(X, np.ones(3 * X.shape[0]), [("TET_NH", tets, PARAMS["TET_NH"])], device_id=-1)
    s.initialize()
    with pytest.raises(pkg.AdmmHipError, match="error 2"):
        s.energy()
    with pytest.raises(pkg.AdmmHipError, match="error 2"):
        s.batch_energy(0)
    assert s.energy_scale(0).shape == (6,) and np.allclose(s.energy_scale(0), H ** 3 / 6.0, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def sized_system(kind):
    """one context whose batches are all of `kind`, with 1, 63, 64, 65 and 270 elements"""
    mg = _pkg().meshgen
    if kind in TET_KINDS:
        X, elems = mg.bar(*BAR, h=H)
    else:
        X, tris, hinges, edges = cloth_mesh()
        elems = tris if kind in TRI_KINDS else (hinges if kind == "BEND" else edges)
        elems = np.tile(elems, (3, 1))
    assert elems.shape[0] >= 270
    forces = [(kind, elems[:n], PARAMS[kind]) for n in SIZES]
    s = build_system(X, np.ones(3 * X.shape[0]), forces)
    s.initialize()
    return s


@gpu
@pytest.mark.parametrize("kind", EVALUATED)
def test_batch_energy_dx_is_bitwise_energy_query(pkg, kind):
    s = sized_system(kind)
    inp = inputs(kind)
    inp = np.roll(inp, inp.shape[0] - 4096, axis=0)      # the hand-made cases first: every batch of more than a few elements has its infinite ones
    any_inf = False
    for b, n in enumerate(SIZES):
        dx = np.ascontiguousarray(inp[:n] if n > 1 else inp[40:41])
        rest = s.read_rest(b)["rest"]
        want = pkg.energy_query(kind, dx, PARAMS[kind], rest, s.energy_scale(b))
        buf = np.full(n + 3, -12345.0)
        got = s.batch_energy_dx(b, dx, out=buf[:n])
        assert np.all(buf[n:] == -12345.0), (kind, n, "wrote past per_elem")
        assert _same_bits(got, want), (kind, n, np.nonzero(_bits(got) != _bits(want))[0][:8])
        assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any()
        any_inf |= bool(np.isinf(got).any())
        # the batch's own state is untouched by the override: the gathered energies are still those of the rest positions
        tot, per, ninf = s.batch_energy(b)
        assert per.shape == (n,) and ninf == int((~np.isfinite(per)).sum())
    assert any_inf == (kind in ("TET_NH", "TRI_FUNG"))


@pytest.fixture(scope="module")
def mixed(pkg):
    X, M3, forces = mixed_forces(PARAMS)
    s = build_system(X, M3, forces)
    s.initialize()
    x = deform(X, fold=True)
    s.m_x = x.ravel()
    v = 0.1 * np.cos(np.arange(x.size, dtype=np.float64))
    s.m_v = v
    return dict(s=s, X=X, M3=M3, forces=forces, x=x, v=v)


@gpu
def test_gather_path_is_bitwise_energy_query(pkg, mixed):
    s, forces, x, X = mixed["s"], mixed["forces"], mixed["x"], mixed["X"]
    kinds_seen = set()
    for b, (kind, idx, _) in enumerate(forces):
        tot, per, ninf = s.batch_energy(b)
        if kind == "COLLISION":
            assert tot == 0.0 and ninf == 0 and not per.any()
            continue
        want = expected_batch_energy(s, b, kind, idx, x, host=X)
        assert per.shape == want.shape
        assert _same_bits(per, want), (b, kind, np.nonzero(_bits(per) != _bits(want))[0][:8])
        assert ninf == int(np.isinf(want).sum())
        kinds_seen.add(kind)
    assert kinds_seen == set(EVALUATED) | {"ANCHOR"}
    assert mixed["forces"][0][0] == "TET_NH" and s.batch_energy(0)[2] > 0      # the fold inverts tets of the first batch


@gpu
def test_totals(pkg, mixed, monkeypatch):
    s, forces = mixed["s"], mixed["forces"]
    e1 = s.energy()
    e2 = s.energy()
    for k in e1:
        assert _same_bits([e1[k]], [e2[k]]) if isinstance(e1[k], float) else e1[k] == e2[k], k
    elastic = 0.0; anchor = 0.0; n_inf = 0
    for b, (kind, idx, _) in enumerate(forces):
        tot, per, ninf = s.batch_energy(b)
        fin = per[np.isfinite(per)]
        assert abs(tot - math.fsum(fin)) <= per.size * EPS * math.fsum(np.abs(fin)), (kind, tot, math.fsum(fin))
        assert ninf == int((~np.isfinite(per)).sum())
        n_inf += ninf
        if kind == "ANCHOR":
            anchor += tot
        elif kind != "COLLISION":
            elastic += tot
    assert _same_bits([e1["elastic"]], [elastic]) and _same_bits([e1["anchor"]], [anchor])
    assert e1["n_infinite"] == n_inf and n_inf > 0
    assert e1["batches_skipped"] == 1
    assert e1["elastic"] > 0.0 and e1["anchor"] > 0.0 and e1["kinetic"] > 0.0
    # the node terms against their definitions (any summation order: n eps of the absolute sum)
    x, v, m3 = mixed["x"].ravel(), mixed["v"], mixed["M3"]
    nn = x.size // 3
    kin = 0.5 * math.fsum(m3 * v * v)
    grav = -math.fsum(m3 * np.tile(G, nn) * x)
    assert abs(e1["kinetic"] - kin) <= nn * EPS * kin
    assert abs(e1["gravity"] - grav) <= nn * EPS * math.fsum(np.abs(m3 * np.tile(G, nn) * x))
    # a context created under other launch knobs returns the same bits
    monkeypatch.setenv("ADMM_HIP_TPB", "16"); monkeypatch.setenv("ADMM_HIP_LOCAL_MULTI", "0"); monkeypatch.setenv("ADMM_HIP_PRERED", "0")
    t = build_system(mixed["X"], mixed["M3"], forces)
    t.initialize()
    t.m_x = mixed["x"].ravel(); t.m_v = mixed["v"]
    e3 = t.energy()
    for k in e1:
        assert _same_bits([e1[k]], [e3[k]]) if isinstance(e1[k], float) else e1[k] == e3[k], k
    for b in range(len(forces)):
        assert _same_bits(s.batch_energy(b)[1], t.batch_energy(b)[1]) and _same_bits([s.batch_energy(b)[0]], [t.batch_energy(b)[0]])


@gpu
def test_gravity_honours_index_subsets_and_skips_wind(pkg):
    mg = pkg.meshgen
    X, tets = mg.bar(*BAR, h=H)
    m = mg.lumped_tet_mass(X, tets, 1000.0)
    s = build_system(X, np.repeat(m, 3), [("TET_NH", tets, PARAMS["TET_NH"])], gravity=None)
    sub = np.array([3, 70, 5, 95, 64], dtype=np.int32)
    s.add_explicit(pkg.EXPLICIT["CONST"], (0.0, -9.8, 0.0))
    s.add_explicit(pkg.EXPLICIT["CONST"], (1.5, 0.0, -2.0), sub)
    s.add_explicit(pkg.EXPLICIT["WIND"], (1.0, 0.0, 0.0), mg.tet_surface(tets)[:10])
    s.initialize()
    x = deform(X)
    s.m_x = x.ravel()
    terms = list(m[:, None] * np.array([0.0, -9.8, 0.0]) * x) + list(m[sub, None] * np.array([1.5, 0.0, -2.0]) * x[sub])
    want = -math.fsum(np.ravel(terms))
    got = s.energy()["gravity"]
    assert abs(got - want) <= len(terms) * 3 * EPS * math.fsum(np.abs(np.ravel(terms))), (got, want)
    assert abs(got - want) < 1e-3 * abs(m[sub].sum() * 1.5 * H)      # the subset's share is far above the bound: it is not dropped


@gpu
def test_free_fall(pkg):
    mg = pkg.meshgen
    X, tets = mg.bar(*BAR, h=H)
    m = mg.lumped_tet_mass(X, tets, 1000.0)
    s = build_system(X, np.repeat(m, 3), [("TET_NH", tets, [1e5, 1e5, 5])])
    s.initialize()
    frames = 3
    for _ in range(frames):
        s.step(5)
    e = s.energy()
    Mtot = math.fsum(m)
    g = 9.8
    kin = 0.5 * Mtot * (frames * DT * g) ** 2
    x = s.m_x.reshape(-1, 3)
    ycm = math.fsum(m * x[:, 1]) / Mtot
    grav = Mtot * g * ycm      # -M g . x_cm with g = (0, -9.8, 0)
    print("free fall: kinetic %.17g (closed form %.17g), gravity %.17g (closed form %.17g), elastic %.3e" % (e["kinetic"], kin, e["gravity"], grav, e["elastic"]))
    assert abs(e["kinetic"] - kin) <= 1e-9 * kin
    assert abs(e["gravity"] - grav) <= 1e-9 * abs(grav)
    V = BAR[0] * BAR[1] * BAR[2] * H ** 3
    assert 0.0 <= abs(e["elastic"]) <= tets.shape[0] * EPS * 1e5 * V
    assert e["anchor"] == 0.0 and e["n_infinite"] == 0 and e["batches_skipped"] == 0


def stretched_bar(material, objective=False):
    """the bar stretched by 1.2 along its axis, its k = 0 face anchored at the rest positions"""
    mg = _pkg().meshgen
    X, tets = mg.bar(*BAR, h=H)
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    if material == "NH":
        forces = [("TET_NH", tets, [1e5, 1e5, 5])]
    else:
        forces = [("TET_LINEAR", tets, PARAMS["TET_LINEAR"]), ("TET_VOLUME", tets, PARAMS["TET_VOLUME"])]
    forces.append(("ANCHOR", mg.bar_anchor_nodes(BAR[0], BAR[1]), [-1.0, 1.0]))
    s = build_system(X, m3, forces)
    s.initialize()
    x0 = X * np.array([1.0, 1.0, 1.2])
    s.m_x = x0.ravel()
    if objective:
        s.enable_objective()
    return s, x0.ravel(), m3, forces


@gpu
@pytest.mark.parametrize("path", ["dense", "sweep"])
@pytest.mark.parametrize("material", ["NH", "LINEAR+VOLUME"])
def test_objective_history(pkg, monkeypatch, path, material):
    if path == "sweep":
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    K = 6
    s, x0, m3, forces = stretched_bar(material, objective=True)
    assert s.info()["dense_solve"] == (1 if path == "dense" else 0)
    s.step(K)
    inertia, elastic, n = s.objective()
    assert n == K and inertia.size == K and elastic.size == K
    nn = x0.size // 3
    xbar = x0 + DT * (0.0 + DT * np.tile(G, nn))
    c = 1.0 / (2.0 * DT * DT)
    for k in range(1, K + 1):
        t, _, _, _ = stretched_bar(material)
        t.step(k)
        e = t.energy()
        absum = sum(math.fsum(np.abs(t.batch_energy(b)[1])) for b, f in enumerate(forces) if f[0] != "ANCHOR")
        assert e["n_infinite"] == 0
        assert abs(elastic[k - 1] - e["elastic"]) <= 270 * EPS * absum, (k, elastic[k - 1], e["elastic"])
        xk = t.m_x
        want = c * math.fsum(m3 * (xk - xbar) ** 2)
        # the terms of m (x - x_bar)^2 expanded, m x^2 - 2 m x x_bar + m x_bar^2, in absolute value: the difference cancels
        absum = c * math.fsum(m3 * (np.abs(xk) + np.abs(xbar)) ** 2)
        assert abs(inertia[k - 1] - want) <= nn * EPS * absum, (k, inertia[k - 1], want)
        assert inertia[k - 1] > 0.0 and elastic[k - 1] > 0.0
    print("%s / %s: objective per iteration %s" % (material, path, inertia + elastic))
    # an early exit ends both histories where the loop ends
    u, _, _, _ = stretched_bar(material, objective=True)
    u.set_tolerance(1e30, 1e30, 2)
    u.step(K)
    i2, e2, n2 = u.objective()
    r, sres, nres = u.residuals()
    assert n2 == nres == 2 and i2.size == e2.size == r.size == 2
    assert _same_bits(i2, inertia[:2]) and _same_bits(e2, elastic[:2])


@gpu
def test_no_side_effects(pkg):
    X, M3, forces = mixed_forces(PARAMS)
    runs = {}
    for mode in ("plain", "energy", "objective"):
        s = build_system(X, M3, forces)
        s.initialize()
        s.m_x = deform(X).ravel()
        if mode == "objective":
            s.enable_objective()
        for f in range(10):
            s.step(4)
            if mode == "energy" and f % 2 == 1:
                s.energy()
                for b in range(len(forces)):
                    s.batch_energy(b)
        runs[mode] = (_state(s, forces), s.graph_state())
    for a, b in zip(runs["plain"][0], runs["energy"][0]):
        assert _same_bits(a, b)
    gp, ge, go = runs["plain"][1], runs["energy"][1], runs["objective"][1]
    assert gp == ge, (gp, ge)      # the same graphs and the same number of launches: no energy call dropped one
    assert gp["iter_graph"] and gp["frame_graph_iters"] == 4 and gp["graph_launches"] >= 9, gp      # the frame graph of four iterations, kept and launched
    assert _same_bits(runs["plain"][0][0], runs["objective"][0][0]) and _same_bits(runs["plain"][0][1], runs["objective"][0][1])
    assert go["graph_launches"] == 0      # with the objective on the loop runs eagerly


@gpu
def test_shards(pkg, monkeypatch):
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DENSE_MAX", "0")
    monkeypatch.setenv("ADMM_HIP_LEAF", "16")
    mg = pkg.meshgen
    dims = (3, 3, 12)
    X, tets = mg.bar(*dims, h=H)
    m3 = np.repeat(mg.lumped_tet_mass(X, tets, 1000.0), 3)
    forces = [("TET_NH", tets[:300], PARAMS["TET_NH"]), ("TET_STVK", tets[300:], PARAMS["TET_STVK"]), ("ANCHOR", mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0])]
    one = build_system(X, m3, forces)
    one.initialize()
    world = 2
    shards = [build_system(X, m3, forces, rank=r, world=world) for r in range(world)]
    for sh, h in zip(shards, _thread_allreduce_hooks(world)):
        sh.set_shard_mode("subtree"); sh.set_allreduce(h)
    pkg.initialize_together(shards)
    x = deform(X)
    v = 0.1 * np.cos(np.arange(x.size, dtype=np.float64))
    for s in [one] + shards:
        s.m_x = x.ravel(); s.m_v = v
    e1 = one.energy()
    es = [s.energy() for s in shards]
    for b, (kind, idx, _) in enumerate(forces):
        tot1, per1, _ = one.batch_energy(b)
        seen = np.zeros(per1.size, dtype=int)
        for s in shards:
            loc = s.local_elements(b)
            _, per, _ = s.batch_energy(b)
            assert _same_bits(per, per1[loc]), (b, kind)
            seen[loc] += 1
        assert (seen == 1).all()
    absum = sum(math.fsum(np.abs(one.batch_energy(b)[1])) for b in range(2))
    assert abs(sum(e["elastic"] for e in es) - e1["elastic"]) <= tets.shape[0] * EPS * absum
    assert min(s.local_elements(0).size + s.local_elements(1).size for s in shards) > 0
    for e in es:
        assert _same_bits([e["kinetic"]], [e1["kinetic"]]) and _same_bits([e["gravity"]], [e1["gravity"]])
    for s in shards:
        with pytest.raises(pkg.AdmmHipError, match="error 4"):
            s.enable_objective()


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
    r = subprocess.run([compile_cpp("scene_energy", pkg), str(inp), str(frames), str(iters)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    en = lines[0].split()
    assert en[0] == "energy"
    s = build_system(X, m3, [("TET_NH", tets, [1e5, 1e5, 5]), ("ANCHOR", anchors, [-1.0, 1.0])])
    s.initialize()
    s.enable_objective()
    for _ in range(frames):
        s.step(iters)
    e = s.energy()
    got = [float.fromhex(v) for v in en[1:5]]
    assert _same_bits(got, [e["kinetic"], e["gravity"], e["elastic"], e["anchor"]]), (got, e)
    assert int(en[5]) == e["n_infinite"] and int(en[6]) == e["batches_skipped"]
    inertia, elastic, n = s.objective()
    assert lines[1] == "objective %d" % iters and n == iters
    hist = np.array([[float.fromhex(v) for v in l.split()[1:3]] for l in lines[2:2 + iters]])
    assert _same_bits(hist[:, 0], inertia) and _same_bits(hist[:, 1], elastic)
