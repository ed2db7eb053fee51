"""Every solve path on systems that are ill-conditioned for a reason Cholesky feels.

tests/test_wide_supernodes.py bounds the forward error in proportion to kappa1, but its only badly conditioned case (i) is so by scaling
alone (equilibrated, its matrix is benign) and passes with orders of slack.  The product replaces every triangular solve by a product
with an inverse (L11^-1 by recursive doubling, L21 L11^-1 panels, (L L^T)^-1 at roots and in the distributed top, A^-1 up to 2 048
nodes): operations whose accuracy depends on conditioning.  Here the same bars are made truly ill-conditioned.

The family ("weak-anchor bar"): make_bar_system(*dims, mu = lam = 1e7, density = d), then the anchor batch's weights times `a` through
set_weights + recompute_weights.  The stiff bar hangs on ever softer anchors and carries ever less mass: the three rigid translations
approach the null space, and no diagonal scaling removes that (kappa1 of D^-1/2 A D^-1/2 stays within 25 % of kappa1 on every rung).
RUNGS lists (d, a); KAPPA the kappa1 measured per shape, which each test asserts within a factor 3, so that a change of the generator
cannot flatten the ladder unseen.  (6, 6, 40): 1.4e4, 3.7e4, 7.5e5, 2.0e6, 2.4e6, 7.5e7, 2.0e8, 1.0e9.

The reference is checkers.SparseReference.solve_ill: refinement with longdouble residuals down to the floor 8 * 2^-64 * kappa1 that the
residual's own precision sets.  test_reference_against_dense_longdouble pins it against a dense Cholesky carried out in np.longdouble
to 1e-3 * 2^-53 * kappa1: the reference is 1000 times more accurate than the bound below.

Bounds.  Forward error |x - x_ref|_inf <= 4 * 2^-53 * kappa1 * |x_ref|_inf; normwise backward error (longdouble residual) <= 1e-14.
Where the host sweeps run over the device's panels, the two solutions share one factor and differ by the rounding of two sweeps, each
amplified by at most kappa1: they agree to max(1e-12, 4 * 2^-53 * kappa1) max|x|.

Calibration (CPU, the library's host path: host factorization + debug_panel_solve_host), forward error / (2^-53 kappa1), largest
over the three right-hand sides, per rung:
    (7, 7, 31) default knobs    0.90 0.90 0.95 0.68 1.07 1.07 1.04 1.06
    (6, 6, 40) LEAF=16          0.87 0.88 0.95 0.66 1.08 1.08 1.04 1.05
    (12, 12, 30)                1.06 1.12 1.21 0.89 1.38 1.38 1.29 1.29
    (3, 3, 10)                  0.024 0.045 0.032 0.19 0.10 0.031 0.020 0.063
largest 1.38 (0.34 of the bound), smallest on the three shapes of 2 009 nodes and more 0.66 (0.17 of the bound: the floor of 1/40 of the
bound is asserted there); backward error <= 1.7e-15 everywhere.  The 160-node bar (3, 3, 10) is in case (a) for dense_solve_kernel's
tail loop; with so few unknowns the host path makes only 0.005 to 0.05 of the bound there, so its rows are printed and held to the two
bounds but not to the floor.

The GPU cases run the rungs at kappa1 ~ 1e4, 1e6 and 1e8 (GPU_RUNGS) with the three right-hand sides of checkers.solve_rhs, and each
asserts from info() or the ADMM_HIP_VERBOSE plan that it ran the path it exists for.
"""
import threading

import numpy as np
import pytest

import checkers
from test_wide_supernodes import BWD_ERR_TOL, SWEEP_TOL, plan, set_env

EPS = 2.0 ** -53
FWD_C = 4.0            # forward error <= FWD_C * EPS * kappa1: the host path makes up to 1.4; the rest allows for another summation order
FLOOR = 1.0 / 40.0     # the host path makes at least this share of the bound: the bound binds
STIFF = dict(mu=1e7, lam=1e7)
RUNGS = [(100.0, 1.0), (100.0, 0.1), (100.0, 0.01), (10.0, 0.01), (1.0, 0.01), (1.0, 1e-3), (0.1, 1e-3), (0.1, 1e-4)]      # (density, anchor weight x)
GPU_RUNGS = (0, 2, 6)  # kappa1 ~ 1e4, ~1e6, ~1e8
KAPPA = {               # kappa1 measured per shape and rung (asserted within a factor 3)
    (7, 7, 31): [8.0e3, 2.6e4, 6.7e5, 1.6e6, 1.9e6, 6.7e7, 1.6e8, 9.8e8],
    (3, 3, 10): [1.3e3, 7.8e3, 4.6e5, 6.3e5, 6.6e5, 4.6e7, 6.3e7, 1.2e9],
    (6, 6, 40): [1.4e4, 3.7e4, 7.5e5, 2.0e6, 2.4e6, 7.5e7, 2.0e8, 1.0e9],
    (12, 12, 30): [6.8e3, 2.5e4, 6.2e5, 1.6e6, 1.8e6, 6.2e7, 1.6e8, 8.9e8],
    (6, 6, 64): [3.4e4, 6.9e4, 8.4e5, 2.9e6, 3.8e6, 8.3e7, 2.9e8, 1.0e9],
    (3, 3, 20): [4.6e3, 1.7e4, 6.7e5, 1.2e6, 1.3e6, 6.7e7, 1.2e8, 1.3e9],
}
SMALL = {"ADMM_HIP_LEAF": "16", "ADMM_HIP_DENSE_MAX": "0"}
SPARSE = {"ADMM_HIP_DENSE_MAX": "0"}
TREES = {"a": ((7, 7, 31), {}), "a_small": ((3, 3, 10), {}), "b": ((6, 6, 40), SMALL), "c": ((12, 12, 30), SPARSE)}


# ---------------------------------------------------------------- the family ----
class Family:
    """the references of the weak-anchor bars, built once: one oracle per (shape, density), one factorization per rung"""

    def __init__(self, pkg):
        self.pkg, self.base, self.refs, self.w = pkg, {}, {}, {}

    def ref(self, dims, rung):
        """-> (SparseReference, x, m3) of rung `rung` on shape `dims`; its kappa1 asserted within a factor 3 of KAPPA"""
        d, a = RUNGS[rung]
        if (dims, rung) not in self.refs:
            if (dims, d) not in self.base:
                self.base[dims, d] = checkers.bar_reference(self.pkg.meshgen, dims, density=d, **STIFF)
            ref0, x, m3 = self.base[dims, d]
            w = np.array(ref0.w0, dtype=np.float64)
            w[6 * dims[0] * dims[1] * dims[2]:] *= a      # tets first, then the anchors (the oracle's force order)
            self.refs[dims, rung] = (ref0.with_weights(w), x, m3)
            self.w[dims, rung] = w
        ref = self.refs[dims, rung][0]
        want = KAPPA[dims][rung]
        assert want / 3.0 <= ref.kappa1 <= 3.0 * want, ("the ladder moved", dims, rung, ref.kappa1, want)
        return self.refs[dims, rung]

    def weights(self, dims, rung):
        """the per-force weights of the rung's reference (tets, then anchors)"""
        self.ref(dims, rung)
        return self.w[dims, rung]


@pytest.fixture(scope="module")
def fam(pkg):
    return Family(pkg)


def weaken_anchors(s, fam, dims, rung):
    """the anchor batch's weights x a through set_weights (recompute_weights is the caller's: a collective call across shards); the
    library's and the oracle's weights agree bit for bit"""
    w = s.read_rest(1)["weight"] * RUNGS[rung][1]
    assert np.array_equal(w, fam.weights(dims, rung)[-w.size:])
    s.set_weights(1, w)
    return w


def weak_anchor_bar(pkg, fam, dims, rung, device_id=0):
    s = pkg.make_bar_system(*dims, density=RUNGS[rung][0], device_id=device_id, **STIFF)
    s.initialize()
    weaken_anchors(s, fam, dims, rung)
    s.recompute_weights()
    return s


def check_solves(s, ref, x, m3, host_sweeps=True, solve=None, seed=7):
    """test_wide_supernodes.check_solves at this module's bounds: forward error, longdouble backward error, host sweeps over the
    device's panels, bitwise reproducibility -> the largest forward error / (EPS kappa1)"""
    solve = solve or s.solve_only
    worst = 0.0
    for i, b in enumerate(checkers.solve_rhs(seed, x, m3)):
        xr, _, _, _ = ref.solve_ill(b)
        xs = solve(b)
        assert np.isfinite(xs).all(), i
        ratio = float(np.abs(xs - xr).max() / np.abs(xr).max()) / (EPS * ref.kappa1)
        eta = ref.backward_error(xs, b)
        print("kappa1 %.3g rhs %d: forward error %.3g x 2^-53 kappa1, backward error %.2g" % (ref.kappa1, i, ratio, eta))
        worst = max(worst, ratio)
        assert ratio <= FWD_C, ("forward error", i, ratio, ref.kappa1, "worst dof", int(np.argmax(np.abs(xs - xr))))
        assert eta <= BWD_ERR_TOL, ("backward error", i, eta, ref.kappa1)
        if host_sweeps:
            xh = s.debug_panel_solve_host(b)
            dh = float(np.abs(xh - xs).max() / np.abs(xs).max())
            assert dh <= max(SWEEP_TOL, FWD_C * EPS * ref.kappa1), ("host sweeps over the device's panels", i, dh, ref.kappa1)
        assert np.array_equal(solve(b), xs), ("not bitwise reproducible", i)
    return worst


def built(pkg, fam, monkeypatch, capfd, dims, env, rung):
    """the weak-anchor bar under `env` with its sweep plan -> (system, levels, roots)"""
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    set_env(monkeypatch, env)
    capfd.readouterr()
    s = weak_anchor_bar(pkg, fam, dims, rung)
    levels, roots, _ = plan(capfd.readouterr().err)
    return s, levels, roots


# ---------------------------------------------------------------- CPU: the reference itself ----
def dense_longdouble_solve(A, B, steps=2):
    """X = A^-1 B by a dense Cholesky carried out in np.longdouble (right-looking, one vectorised column per step), two substitution
    sweeps and `steps` steps of refinement in the same precision.  A dense symmetric positive definite, B [n][m]."""
    ld = np.longdouble
    A = np.asarray(A, dtype=ld); B = np.asarray(B, dtype=ld)
    n = A.shape[0]
    L = np.tril(A)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
        c = L[j + 1:, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(c, c))

    def sub(R):
        Y = np.array(R, dtype=ld)
        for j in range(n):
            Y[j] /= L[j, j]
            Y[j + 1:] -= np.outer(L[j + 1:, j], Y[j])
        for j in range(n - 1, -1, -1):
            Y[j] /= L[j, j]
            Y[:j] -= np.outer(L[j, :j], Y[j])
        return Y
    X = sub(B)
    for _ in range(steps):
        X = X + sub(B - A @ X)
    return X


@pytest.mark.parametrize("rung", [5, 7])
def test_reference_against_dense_longdouble(pkg, fam, rung):
    """(3, 3, 20), 336 nodes, kappa1 6.7e7 and 1.3e9: SparseReference.solve_ill = a dense longdouble Cholesky to 1e-3 * 2^-53 * kappa1,
    relative to |x|_inf -- the reference is at least 1000 times more accurate than the bound it serves.  Every force's selector acts on
    the three coordinates alike, so A = A_s (x) I_3 (asserted) and the dense solve is that of the scalar n x n system A_s with the
    coordinates of a right-hand side as columns.  Measured: the two differ by 0.0014 to 0.012 of the allowance, and the reference's
    last correction (two steps each) is 7.1e-14 |x| at most at kappa1 6.7e7 and 1.1e-12 |x| at 1.3e9."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    dims = (3, 3, 20)
    ref, x, m3 = fam.ref(dims, rung)
    assert ref.kappa1 >= 1e7
    A = ref.A.toarray()
    n = A.shape[0] // 3
    As = A[0::3, 0::3]
    assert n == 336 and np.array_equal(A, np.kron(As, np.eye(3))) and np.array_equal(As, As.T)
    B = checkers.solve_rhs(7, x, m3)
    X = dense_longdouble_solve(As, np.concatenate([b.reshape(n, 3) for b in B], axis=1))
    for i, b in enumerate(B):
        xr, _, steps, corr = ref.solve_ill(b)
        xd = X[:, 3 * i:3 * i + 3].ravel()
        diff = float(np.abs(xr.astype(np.longdouble) - xd).max() / np.abs(xd).max())
        allow = 1e-3 * EPS * ref.kappa1
        print("kappa1 %.3g rhs %d: |x_ref - x_dense| = %.3g |x| = %.3g of the allowance; %d steps, last correction %.2g |x|" % (ref.kappa1, i, diff, diff / allow, steps, corr))
        assert diff <= allow, (i, diff, allow)
        assert corr <= allow, (i, corr, allow)      # what is left after the last correction is smaller still


def test_solve_keeps_its_stopping_rule(pkg, fam):
    """the well-conditioned callers' rule is unchanged: solve stops at a correction below 1e-16 |x| (two steps on rung 0) and returns
    three values; kappa1_eq is computed once and not carried over by with_weights"""
    ref, x, m3 = fam.ref((6, 6, 40), 0)
    b = checkers.solve_rhs(7, x, m3)[0]
    xr, res, steps = ref.solve(b)
    assert steps == 2 and ref.backward_error(xr, b) <= 1e-16
    x4 = ref.solve_ill(b)
    assert len(x4) == 4 and np.abs(x4[0] - xr).max() <= 2 * EPS * np.abs(xr).max()
    k = ref.kappa1_eq
    assert 0.5 * ref.kappa1 <= k <= ref.kappa1 * 1.01 and ref.kappa1_eq == k
    other = fam.ref((6, 6, 40), 2)[0]
    assert other.kappa1_eq > 10 * k


# ---------------------------------------------------------------- CPU: calibration on the host path ----
@pytest.mark.parametrize("tree", list(TREES))
def test_host_path_calibrates_the_bound(pkg, fam, monkeypatch, tree):
    """the library's host path (device_id = -1: host factorization, debug_panel_solve_host) on every rung of the ladder, on the trees
    of cases (a) to (c): inside both bounds, and -- on the shapes of 2 009 nodes and more -- at least 1/40 of the forward bound, so the
    bound binds.  The family stays ill-conditioned under equilibration: kappa1_eq >= 0.7 kappa1.  Prints the ratio per rung."""
    dims, env = TREES[tree]
    set_env(monkeypatch, env)
    lo, hi = np.inf, 0.0
    for rung in range(len(RUNGS)):
        ref, x, m3 = fam.ref(dims, rung)
        assert ref.kappa1_eq >= 0.7 * ref.kappa1, (rung, ref.kappa1_eq, ref.kappa1)
        s = weak_anchor_bar(pkg, fam, dims, rung, device_id=-1)
        worst = check_solves(s, ref, x, m3, host_sweeps=False, solve=s.debug_panel_solve_host)
        print("%s rung %d (density %g, anchors x %g): kappa1 %.3g, equilibrated %.3g, host path %.3g x 2^-53 kappa1 = %.3g of the bound"
              % (dims, rung, RUNGS[rung][0], RUNGS[rung][1], ref.kappa1, ref.kappa1_eq, worst, worst / FWD_C))
        if tree != "a_small":
            assert worst >= FLOOR * FWD_C, ("the bound does not bind", rung, worst)
        lo, hi = min(lo, worst), max(hi, worst)
    print("%s: forward error / (2^-53 kappa1) between %.3g and %.3g over the ladder" % (dims, lo, hi))
    assert fam.ref(dims, len(RUNGS) - 1)[0].kappa1 >= 1e8


# ---------------------------------------------------------------- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("rung", GPU_RUNGS)
@pytest.mark.parametrize("dims", [(7, 7, 31), (3, 3, 10)], ids=["2048_nodes", "160_nodes"])
def test_a_dense_inverse(pkg, fam, dims, rung):
    """(a) the explicit inverse (dense_solve_kernel), the path every small scene takes, default knobs: 2 048 nodes (the largest it
    serves) and 160 (its tail loop).  Measured on the MI355X, largest forward error / (2^-53 kappa1) over rungs and right-hand
    sides: 1.04 at 2 048 nodes (the host path's own figure), 0.032 at 160; backward error 1.3e-15 at most."""
    ref, x, m3 = fam.ref(dims, rung)
    s = weak_anchor_bar(pkg, fam, dims, rung)
    assert s.info()["dense_solve"] == 1 and s.info()["n_nodes"] == x.shape[0]
    check_solves(s, ref, x, m3, host_sweeps=False)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", GPU_RUNGS)
@pytest.mark.parametrize("root_inverse", [True, False], ids=["root_inverse", "root_by_sweeps"])
@pytest.mark.parametrize("factor", ["gpu", "host"])
def test_b_small_supernodes(pkg, fam, monkeypatch, capfd, factor, root_inverse, rung):
    """(b) (6, 6, 40) with LEAF=16 DENSE_MAX=0: 135 supernodes of at most 171 columns (one or two doubling rounds for L11^-1), the
    factorization on the device and on the host, the root through its explicit inverse and through the sweeps.  Measured on the
    MI355X: forward error / (2^-53 kappa1) 1.05 at most in all four configurations, backward error 1.1e-15 at most."""
    dims = (6, 6, 40)
    env = dict(SMALL)
    if factor == "host":
        env["ADMM_HIP_FACTOR"] = "host"
    if not root_inverse:
        env["ADMM_HIP_ROOT_INVERSE"] = "0"
    ref, x, m3 = fam.ref(dims, rung)
    s, levels, roots = built(pkg, fam, monkeypatch, capfd, dims, env, rung)
    info = s.info()
    assert info["dense_solve"] == 0 and info["device_factor"] == (1 if factor == "gpu" else 0), info
    assert info["n_supernodes"] > 100 and 64 < info["max_super_cols"] <= 256, info
    assert levels and bool(roots) == root_inverse, (levels, roots)
    check_solves(s, ref, x, m3)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", GPU_RUNGS)
def test_c_many_block_supernodes(pkg, fam, monkeypatch, capfd, rung):
    """(c) (12, 12, 30) with DENSE_MAX=0, default tree, device factorization: a root of more than 256 columns (1 344: at least three
    doubling rounds for its L11^-1, then L^-T L^-1) over supernodes of up to 111 columns.  Measured on the MI355X: forward error /
    (2^-53 kappa1) 1.31 at most (host path on this tree: 1.29 on that rung, 1.38 over the ladder), backward error 1.2e-15 at most."""
    dims = (12, 12, 30)
    ref, x, m3 = fam.ref(dims, rung)
    s, levels, roots = built(pkg, fam, monkeypatch, capfd, dims, SPARSE, rung)
    assert s.info()["device_factor"] == 1 and s.info()["dense_solve"] == 0
    assert any(R["k"] > 256 for R in roots), roots
    check_solves(s, ref, x, m3)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", GPU_RUNGS)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_d_shards(pkg, fam, monkeypatch, capfd, world, rung):
    """(d) (6, 6, 64) with LEAF=16 DENSE_MAX=0 on subtree shards, ranks as threads on one GPU, rank-local factorization: 2 and 4 ranks
    with the distributed top (every rank its rows of the root's inverse), 3 ranks with the replicated top.  The anchors are weakened by
    the collective recompute_weights on every rank; every rank's solve_only against the reference, all ranks bitwise equal.
    Measured on the MI355X: forward error / (2^-53 kappa1) 0.80 at most over the three world sizes, backward error 8.3e-16 at most."""
    from test_sharding import _thread_allreduce_hooks
    dims = (6, 6, 64)
    dist = world != 3
    set_env(monkeypatch, SMALL)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    if dist:
        monkeypatch.setenv("ADMM_HIP_DIST_TOP", "1")
    ref, x, m3 = fam.ref(dims, rung)
    capfd.readouterr()
    ss = [pkg.make_bar_system(*dims, density=RUNGS[rung][0], device_id=0, rank=r, world=world, shard_mode="subtree", **STIFF) for r in range(world)]
    for s, h in zip(ss, _thread_allreduce_hooks(world)):
        s.set_allreduce(h)
    pkg.initialize_together(ss, timeout=300.0)
    _, _, dplan = plan(capfd.readouterr().err)
    for s in ss:
        info = s.info()
        assert info["factor_local"] == 1 and info["device_factor"] == 1 and info["dense_solve"] == 0 and info["dist_top"] == (1 if dist else 0), info
    assert len(dplan) == (world if dist else 0) and all(0 < d["nrows"] < d["k"] for d in dplan), dplan
    for s in ss:
        weaken_anchors(s, fam, dims, rung)
    pkg.call_together(ss, "recompute_weights", timeout=300.0)

    def solve(b):
        out, errs = [None] * world, []

        def run(r):
            try:
                out[r] = ss[r].solve_only(b)
            except BaseException as e:  # noqa: BLE001
                errs.append((r, repr(e)))
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]; [t.join(timeout=300) for t in th]
        assert not errs and all(o is not None for o in out), errs
        for r in range(1, world):
            assert np.array_equal(out[r], out[0]), ("ranks differ", r)
        return out[0]
    check_solves(ss[0], ref, x, m3, host_sweeps=False, solve=solve)


def tet_linear_frames(pkg, fam, env, monkeypatch, dims, rung, n=3, iters=8):
    """n frames of the rung's bar with corotational tets of the same stiffness (TET_LINEAR: the same weights, so the same A, and no
    truncated minimiser), run twice -> the frames, asserted finite and bitwise reproducible"""
    set_env(monkeypatch, env)
    mg = pkg.meshgen
    x, t = mg.bar(*dims)
    runs = []
    for _ in range(2):
        s = pkg.System(device_id=0); s.set_timestep(0.04)
        s.add_nodes(x.ravel(), np.repeat(mg.lumped_tet_mass(x, t, RUNGS[rung][0]), 3))
        s.add_forces(pkg.KIND["TET_LINEAR"], t, [STIFF["mu"]])
        s.add_forces(pkg.KIND["ANCHOR"], mg.bar_anchor_nodes(dims[0], dims[1]), [-1.0, 1.0])
        s.add_gravity([0.0, -9.8, 0.0])
        s.initialize()
        w = np.concatenate([s.read_rest(0)["weight"], weaken_anchors(s, fam, dims, rung)])
        assert np.array_equal(w, fam.weights(dims, rung))      # the rung's own system
        s.recompute_weights()
        xs = []
        for _ in range(n):
            s.step(iters); xs.append(s.m_x.copy())
        runs.append((xs, s.info()["device_factor"]))
    for f in range(n):
        assert np.isfinite(runs[0][0][f]).all(), f
        assert np.array_equal(runs[0][0][f], runs[1][0][f]), ("frame not bitwise reproducible", env, f)
    for k in env:
        monkeypatch.delenv(k)
    return runs[0]


@pytest.mark.gpu
def test_e_frames(pkg, fam, monkeypatch):
    """(e) rung 2 of case (b) (kappa1 7.5e5) over three frames of 8 iterations with corotational tets: the device factorization against
    ADMM_HIP_FACTOR=host.  Both finite, each bitwise reproducible; their difference is printed and not bounded (no reference exists
    for it).  Measured on the MI355X: 7.9e-14, 4.1e-14, 5.8e-14 at max|x| = 2."""
    dims, rung = (6, 6, 40), 2
    dev, fdev = tet_linear_frames(pkg, fam, SMALL, monkeypatch, dims, rung)
    host, fhost = tet_linear_frames(pkg, fam, dict(SMALL, ADMM_HIP_FACTOR="host"), monkeypatch, dims, rung)
    assert fdev == 1 and fhost == 0
    for f in range(len(dev)):
        print("frame %d: |x_device_factor - x_host_factor| = %.3g, max|x| %.3g" % (f + 1, float(np.abs(dev[f] - host[f]).max()), float(np.abs(dev[f]).max())))
