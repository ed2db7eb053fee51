"""The global step at the shapes where its kernels branch, against an independent extended-precision solve.

Every other test that moves the sweep kernels or the elimination tree runs on bars of at most 12x12x30, where no block item
needs a second column chunk, no front needs a second row chunk in the backward kernel and no root a second chunk in its
product.  Here a 24x24x60 Neo-Hookean bar (38 125 nodes, 207 360 tets) reaches them:

  * default tree (tree search: eight-way nodes): a level of 8 supernodes of up to 908 columns and fronts of up to 1 967 rows,
    a 3 503-column root (root_gather + a two-chunk root_product, odd last chunk);
  * ADMM_HIP_TREE_SEARCH=0 MERGE=0: a binary tree with a 1 953-column root (fused, one chunk, odd k);
    with MERGE_ROOT=0 as well the two top separators of 651 columns stay separate supernodes (fronts of 1 302 rows).

Every case asserts from the sweep plan that admm_hip prints under ADMM_HIP_VERBOSE (upload.inc, one line per level and pass,
one per root) that it reached the path it exists for, then solves the three right-hand sides of checkers.solve_rhs and checks

  * forward error: |x - x_ref|_inf <= tol(kappa1) |x_ref|_inf, x_ref = checkers.SparseReference (the oracle's D, W and masses,
    SuperLU, iterative refinement with longdouble residuals).  tol = 1e-12 up to kappa1 = 2e4 (the 24x24x60 bar: 1.6e4) and
    proportional to kappa1 beyond; the library's host path (host factorization + host sweeps) is 2e-13 off at most on this bar;
  * residual, in longdouble against the oracle-assembled A: the normwise backward error |b - A x| / (|A| |x| + |b|) <= 1e-14 for
    every right-hand side (host path: <= 2e-16), and |b - A x| <= 1e-13 |b| for the white-noise one (host path: 2e-14).  The
    smooth right-hand side solves to x ~ positions with |A| |x| >> |b|: there |b - A x| / |b| is ~5e-14 for x_ref rounded to
    doubles and ~2e-12 for the host path, so a bound relative to |b| alone does not fit it;
  * host sweeps: debug_panel_solve_host(b) over the device's own panels = x to 1e-12 max|x| (sweep kernels vs factorization);
  * reproducibility: two solves of one b are bitwise equal.

Cases that move a knob also run a few frames of the same bar with corotational tets (TET_LINEAR, no truncated minimiser)
against the default build: 1e-9, as tests/test_knobs.py.  The references are built once per module (~20-35 s each).
"""
import re
import threading

import numpy as np
import pytest

import checkers

DIMS = (24, 24, 60)
FWD_TOL, KAPPA_BASE = 1e-12, 2e4
RES_TOL, BWD_ERR_TOL, SWEEP_TOL = 1e-13, 1e-14, 1e-12
BINARY = {"ADMM_HIP_TREE_SEARCH": "0", "ADMM_HIP_MERGE": "0"}
BINARY_SPLIT_TOP = dict(BINARY, ADMM_HIP_MERGE_ROOT="0", ADMM_HIP_ROOT_INVERSE="0")
NW8 = {"ADMM_HIP_FWD_NW16_TILES": "0", "ADMM_HIP_FWD_NW4": "0", "ADMM_HIP_FWD_NW8": "100000"}
NW4 = {"ADMM_HIP_FWD_NW16_TILES": "0", "ADMM_HIP_FWD_NW4": "100000"}
STIFF = dict(mu=1e7, lam=1e7, density=100.0)
STIFF_SOFT = 1e-3       # case (i): the weights of the tets in the upper half of the bar (in z) scaled by this
EQ_C, EQ_EPS = 4.0, 2.0 ** -53      # case (i): forward error <= EQ_C * EQ_EPS * kappa1_eq, the condition number of the equilibrated matrix


def fwd_tol(kappa1):
    """forward-error bound: 1e-12 up to kappa1 = 2e4, proportional to kappa1 beyond (the rounding of the solve is amplified by kappa)"""
    return FWD_TOL * max(1.0, kappa1 / KAPPA_BASE)


# ---------------------------------------------------------------- references (once per module) ----
@pytest.fixture(scope="module")
def ref_nh(pkg):
    return checkers.bar_reference(pkg.meshgen, DIMS)


def stiff_weights(pkg, w):
    """case (i): a uniform bar's kappa1 is bounded by its stiffness matrix's (mu = lam = 1e7 at density 100: 2.4e4 against 1.6e4); a
    1e-3 contrast of the weights (1e-6 of the stiffness) between the two halves of the bar takes it to ~7e6"""
    x, t = pkg.meshgen.bar(*DIMS)
    zc = x[t].mean(axis=1)[:, 2]
    w = np.array(w, dtype=np.float64)
    w[:t.shape[0]][zc > zc.mean()] *= STIFF_SOFT
    return w


@pytest.fixture(scope="module")
def ref_stiff(pkg):
    ref, x, m3 = checkers.bar_reference(pkg.meshgen, DIMS, **STIFF)
    return ref.with_weights(stiff_weights(pkg, ref.w0)), x, m3


def stiff_bar(pkg, device_id=0):
    s = bar(pkg, device_id=device_id, **STIFF)
    nt = s.n_tets
    w = stiff_weights(pkg, np.concatenate([s.read_rest(0)["weight"], s.read_rest(1)["weight"]]))
    s.set_weights(0, w[:nt]); s.set_weights(1, w[nt:]); s.recompute_weights()
    return s


def edited_weights(w):
    """anchors at half their weight, every third tet at twice its weight (w: tets then anchors, the oracle's force order)"""
    nt = 6 * DIMS[0] * DIMS[1] * DIMS[2]
    w = np.array(w, dtype=np.float64)
    w[:nt:3] *= 2.0
    w[nt:] *= 0.5
    return w


@pytest.fixture(scope="module")
def ref_edited(ref_nh):
    ref, x, m3 = ref_nh
    return ref.with_weights(edited_weights(ref.w0)), x, m3


# ---------------------------------------------------------------- helpers ----
def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def bar(pkg, device_id=0, **kw):
    s = pkg.make_bar_system(*DIMS, device_id=device_id, **kw)
    s.initialize()
    return s


def plan(err):
    """the sweep plan lines of admm_hip (upload.inc) -> (levels, roots, dist): dicts of the printed fields"""
    levels, roots, dist = [], [], []
    for m in re.finditer(r"admm_hip: plan (own|top) level (\d+): fwd wave (\d+) block (\d+) big_nw (\d+) kmax (\d+) chunks (\d+) \| "
                         r"bwd cw (\d+) nw (\d+) items (\d+) fmax (\d+) rchunks (\d+) \| cg4 (\d)", err):
        g = m.groups()
        levels.append(dict(pass_=g[0], level=int(g[1]), wave=int(g[2]), block=int(g[3]), big_nw=int(g[4]), kmax=int(g[5]), chunks=int(g[6]),
                           cw=int(g[7]), nw=int(g[8]), items=int(g[9]), fmax=int(g[10]), rchunks=int(g[11]), cg4=int(g[12])))
    for m in re.finditer(r"admm_hip: plan (own|top) level (\d+): root k (\d+) (fused|gather) chunks (\d+)", err):
        g = m.groups()
        roots.append(dict(pass_=g[0], level=int(g[1]), k=int(g[2]), fused=g[3] == "fused", chunks=int(g[4])))
    for m in re.finditer(r"admm_hip: plan dist-top rank (\d+): root k (\d+) rows (\d+)\.\.(\d+) nrows (\d+) chunks (\d+)", err):
        g = [int(v) for v in m.groups()]
        dist.append(dict(rank=g[0], k=g[1], r0=g[2], r1=g[3], nrows=g[4], chunks=g[5]))
    return levels, roots, dist


def built_with_plan(pkg, monkeypatch, capfd, env, **kw):
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    set_env(monkeypatch, env)
    capfd.readouterr()
    s = bar(pkg, **kw)
    levels, roots, dist = plan(capfd.readouterr().err)
    assert levels, "no sweep plan printed"
    return s, levels, roots


def check_solves(s, ref, x, m3, host_sweeps=True, seed=7):
    """forward error, longdouble residual, host sweeps over the device's panels, bitwise reproducibility; -> the forward errors"""
    B = checkers.solve_rhs(seed, x, m3)
    tol = fwd_tol(ref.kappa1)
    errs = []
    for i, b in enumerate(B):
        xr, _, _ = ref.solve(b)
        xs = s.solve_only(b)
        assert np.isfinite(xs).all(), i
        err = float(np.abs(xs - xr).max() / np.abs(xr).max())
        errs.append(err)
        assert err <= tol, ("forward error", i, err, tol, "worst dof", int(np.argmax(np.abs(xs - xr))))
        eta = ref.backward_error(xs, b)
        assert eta <= BWD_ERR_TOL, ("backward error", i, eta)
        if i == 0:
            res = float(np.abs(ref.residual(xs, b)).max() / np.abs(b).max())
            assert res <= RES_TOL, ("residual", i, res)
        if host_sweeps:
            xh = s.debug_panel_solve_host(b)
            assert np.abs(xh - xs).max() <= SWEEP_TOL * np.abs(xs).max(), ("host sweeps over the device's panels", i, float(np.abs(xh - xs).max() / np.abs(xs).max()))
        assert np.array_equal(s.solve_only(b), xs), ("not bitwise reproducible", i)
    print("forward errors %s (tol %.2g, kappa1 %.3g)" % (", ".join("%.2g" % e for e in errs), tol, ref.kappa1))
    return errs


def frames(pkg, env, monkeypatch, n=3, iters=8):
    """a few frames of the same bar with corotational tets (no truncated minimiser) under `env`"""
    set_env(monkeypatch, env)
    mg = pkg.meshgen
    x, t = mg.bar(*DIMS)
    s = pkg.System(device_id=0); s.set_timestep(0.04)
    s.add_nodes(x.ravel(), np.repeat(mg.lumped_tet_mass(x, t, 1000.0), 3))
    s.add_forces(pkg.KIND["TET_LINEAR"], t, [4000.0])
    s.add_forces(pkg.KIND["ANCHOR"], mg.bar_anchor_nodes(DIMS[0], DIMS[1]), [-1.0, 1.0])
    s.add_gravity([0.0, -9.8, 0.0])
    s.initialize()
    xs = []
    for _ in range(n):
        s.step(iters); xs.append(s.m_x.copy())
    for k in env:
        monkeypatch.delenv(k)
    return xs


@pytest.fixture(scope="module")
def frames_default(pkg):
    mp = pytest.MonkeyPatch()
    try:
        return frames(pkg, {}, mp)
    finally:
        mp.undo()


def check_frames(pkg, env, monkeypatch, frames_default):
    monkeypatch.delenv("ADMM_HIP_VERBOSE", raising=False)
    got = frames(pkg, env, monkeypatch)
    for f in range(len(got)):
        assert np.isfinite(got[f]).all()
        assert np.abs(got[f] - frames_default[f]).max() < 1e-9, (env, f, float(np.abs(got[f] - frames_default[f]).max()))


# ---------------------------------------------------------------- CPU: the reference itself ----
def test_reference_reproduces_the_compiled_reference_solve(pkg):
    """bar100k (16x16x65): the extended-precision reference = the compiled reference's own solver.solve (tests/golden/solve_bar100k.npz)
    at test_solve_parity's 1e-10 bound; the observed agreement is printed (far tighter)."""
    from conftest import golden
    from test_solve_parity import check
    ref, x, m3 = checkers.bar_reference(pkg.meshgen, (16, 16, 65))
    g = golden("solve_bar100k.npz")
    B = checkers.solve_rhs(int(g["seed"]), x, m3)
    X = np.stack([ref.solve(b)[0] for b in B])
    check(g, X)
    st = int(g["stride"])
    print("reference vs solve_bar100k.npz: %s relative" % ", ".join("%.2g" % (np.abs(X[r][::st] - g["x"][r]).max() / float(g["x_max"][r])) for r in range(3)))
    for b in B:
        xr, _, _ = ref.solve(b)
        assert ref.backward_error(xr, b) <= 1e-16


@pytest.mark.parametrize("tree", ["default", "binary"])
def test_host_path_meets_the_bounds(pkg, monkeypatch, ref_nh, tree):
    """the library's host path (host-only context: host factorization, debug_panel_solve_host) on the 24x24x60 bar, default and binary
    tree, against the reference at the GPU cases' bounds -- the calibration of those bounds on hardware-independent arithmetic"""
    if tree == "binary":
        set_env(monkeypatch, BINARY)
    ref, x, m3 = ref_nh
    s = bar(pkg, device_id=-1)
    tol = fwd_tol(ref.kappa1)
    assert 1e4 < ref.kappa1 < KAPPA_BASE
    for b in checkers.solve_rhs(7, x, m3):
        xr, _, _ = ref.solve(b)
        xs = s.debug_panel_solve_host(b)
        err = np.abs(xs - xr).max() / np.abs(xr).max()
        res, eta = np.abs(ref.residual(xs, b)).max() / np.abs(b).max(), ref.backward_error(xs, b)
        print("host path (%s tree): forward %.2g, residual %.2g |b|, backward error %.2g" % (tree, err, res, eta))
        assert err <= tol and eta <= BWD_ERR_TOL
    b = checkers.solve_rhs(7, x, m3)[0]
    assert np.abs(ref.residual(s.debug_panel_solve_host(b), b)).max() <= RES_TOL * np.abs(b).max()


def test_host_path_stiff_meets_the_kappa_rule(pkg, ref_stiff, ref_nh):
    """the badly conditioned bar of case i (mu = lam = 1e7, density 100, weight contrast 1e-3): kappa1 at least 100x the default bar's;
    the host path within fwd_tol(kappa1) and the backward-error bound, and within EQ_C * 2^-53 * kappa1_eq of the equilibrated matrix
    (kappa1_eq 6.4e3; measured 0.0008, 0.008 and 0.24 x 2^-53 kappa1_eq for the three right-hand sides) -- the bound case (i) adds"""
    ref, x, m3 = ref_stiff
    assert ref.kappa1 >= 100 * ref_nh[0].kappa1, (ref.kappa1, ref_nh[0].kappa1)
    s = stiff_bar(pkg, device_id=-1)
    for b in checkers.solve_rhs(7, x, m3):
        xr, _, _ = ref.solve(b)
        xs = s.debug_panel_solve_host(b)
        err = np.abs(xs - xr).max() / np.abs(xr).max()
        eta = ref.backward_error(xs, b)
        print("host path (stiff, kappa1 %.3g): forward %.2g (tol %.2g), backward error %.2g" % (ref.kappa1, err, fwd_tol(ref.kappa1), eta))
        print("  equilibrated kappa1 %.3g: forward error %.3g x 2^-53 kappa1_eq (bound %g)" % (ref.kappa1_eq, err / (EQ_EPS * ref.kappa1_eq), EQ_C))
        assert err <= fwd_tol(ref.kappa1) and eta <= BWD_ERR_TOL
        assert err <= EQ_C * EQ_EPS * ref.kappa1_eq


def test_reference_with_edited_weights(pkg, monkeypatch, ref_edited):
    """the reference rebuilt for edited weights = the library's host path after set_weights + recompute_weights"""
    ref, x, m3 = ref_edited
    s = bar(pkg, device_id=-1)
    nt = s.n_tets
    w = edited_weights(np.concatenate([s.read_rest(0)["weight"], s.read_rest(1)["weight"]]))
    s.set_weights(0, w[:nt]); s.set_weights(1, w[nt:]); s.recompute_weights()
    b = checkers.solve_rhs(7, x, m3)[0]
    xr, _, _ = ref.solve(b)
    assert np.abs(s.debug_panel_solve_host(b) - xr).max() <= fwd_tol(ref.kappa1) * np.abs(xr).max()


# ---------------------------------------------------------------- GPU ----
@pytest.mark.gpu
def test_a_default_tree(pkg, monkeypatch, capfd, ref_nh):
    """(a) default tree: the eight-way level (k 908) through solve_fwd_big_kernel<.,16>; the 3 503-column root through root_gather_kernel
    and a two-chunk root_product_kernel<false, .> (2 048 + 1 455 columns: odd last chunk, pair loads over the padding column)"""
    s, levels, roots = built_with_plan(pkg, monkeypatch, capfd, {})
    assert any(L["big_nw"] == 16 and L["kmax"] > 512 for L in levels), levels
    assert any(not R["fused"] and R["chunks"] == 2 and (R["k"] - 2048) % 2 == 1 for R in roots), roots
    check_solves(s, *ref_nh)


@pytest.mark.gpu
def test_b_nw8_column_chunks(pkg, monkeypatch, capfd, ref_nh, frames_default):
    """(b) solve_fwd_big_kernel<.,8> in two 512-column chunks on the eight-way level (k 908): the chunk loop (second barrier, restaging
    of ts, per-chunk wave split, kneed clipping); the plan line says whether this is the CG2 or the plain staging loop"""
    s, levels, _ = built_with_plan(pkg, monkeypatch, capfd, NW8)
    hit = [L for L in levels if L["big_nw"] == 8 and L["chunks"] >= 2]
    assert hit, levels
    print("NW8 chunked levels:", hit)
    check_solves(s, *ref_nh)
    check_frames(pkg, NW8, monkeypatch, frames_default)


@pytest.mark.gpu
def test_c_nw4_column_chunks(pkg, monkeypatch, capfd, ref_nh, frames_default):
    """(c) solve_fwd_big_kernel<.,4> in two 512-column chunks on the eight-way level (k 908)"""
    s, levels, _ = built_with_plan(pkg, monkeypatch, capfd, NW4)
    assert any(L["big_nw"] == 4 and L["chunks"] >= 2 for L in levels), levels
    check_solves(s, *ref_nh)
    check_frames(pkg, NW4, monkeypatch, frames_default)


@pytest.mark.gpu
def test_d_root_through_the_sweeps(pkg, monkeypatch, capfd, ref_nh, frames_default):
    """(d) ADMM_HIP_ROOT_INVERSE=0 ROOT_DEPTH=3: the 3 503-column root through solve_fwd_big_kernel<.,16> in two 2 048-column chunks and
    through solve_bwd_kernel in four 1 024-row chunks.  (Without a root inverse the tree search keeps the rule-based tree, whose root has
    1 953 columns; ROOT_DEPTH=3 makes the root span the same seven separators as the default tree's.)"""
    env = {"ADMM_HIP_ROOT_INVERSE": "0", "ADMM_HIP_ROOT_DEPTH": "3"}
    s, levels, roots = built_with_plan(pkg, monkeypatch, capfd, env)
    assert not roots
    assert any(L["big_nw"] == 16 and L["chunks"] == 2 and L["kmax"] > 2048 and L["rchunks"] == 4 for L in levels), levels
    check_solves(s, *ref_nh)
    check_frames(pkg, env, monkeypatch, frames_default)


@pytest.mark.gpu
def test_e_binary_tree_cg2_column_chunks(pkg, monkeypatch, capfd, ref_nh):
    """(e) the CG2 (quadruple-list) staging in the chunk loop of solve_fwd_big_kernel<true, 8>.  Scene: the 24x24x60 bar with
    ADMM_HIP_TREE_SEARCH=0 MERGE=0 MERGE_ROOT=0 ROOT_INVERSE=0 -- a binary tree whose two top separators (651 columns, fronts of
    1 302 rows: carries into the root) are NOT the root -- forced to 8 waves per tile: two 512-column chunks on a non-root level"""
    s, levels, roots = built_with_plan(pkg, monkeypatch, capfd, dict(BINARY_SPLIT_TOP, **NW8))
    last = max(L["level"] for L in levels)
    hit = [L for L in levels if L["big_nw"] == 8 and L["chunks"] >= 2 and L["level"] < last and L["fmax"] > L["kmax"]]
    assert hit and all(L["cg4"] == 1 for L in levels), levels
    assert not roots
    check_solves(s, *ref_nh)


BWD_PAIRS = [(4, 2), (4, 4), (4, 8), (4, 16), (2, 4), (2, 8), (2, 16), (1, 4), (1, 8), (1, 16)]


def bwd_env(cw, nw):
    if cw == 4:      # every level "small": four columns per wave, BWD_SMALL_NW waves
        return {"ADMM_HIP_BWD_SMALL_K": "100000", "ADMM_HIP_BWD_SMALL_NW": str(nw)}
    env = {"ADMM_HIP_BWD_SMALL_K": "0", "ADMM_HIP_BWD_NW_MIN_COLS": "0", "ADMM_HIP_BWD_NW": str(nw)}
    env.update(ADMM_HIP_BWD_CW2_MIN="1", ADMM_HIP_BWD_CW2_MAX="100000000") if cw == 2 else env.update(ADMM_HIP_BWD_CW2_MIN="0")
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("cw,nw", BWD_PAIRS)
def test_f_backward_instantiations_on_tall_fronts(pkg, monkeypatch, capfd, ref_nh, cw, nw):
    """(f) solve_bwd_kernel<CW, NWB> for every pair of launch.inc's ADMM_BWD list on a level whose tallest front exceeds 1 024 rows
    (the eight-way level of the default tree: fronts of up to 1 967 rows): two row chunks of the staged vector"""
    s, levels, _ = built_with_plan(pkg, monkeypatch, capfd, bwd_env(cw, nw))
    assert any(L["cw"] == cw and L["nw"] == nw and L["items"] > 0 and L["fmax"] > 1024 and L["rchunks"] >= 2 for L in levels), levels
    check_solves(s, *ref_nh)


@pytest.mark.gpu
def test_g_fused_root_near_the_chunk_size(pkg, monkeypatch, capfd, ref_nh, frames_default):
    """(g) binary tree (ADMM_HIP_TREE_SEARCH=0 MERGE=0): the 1 953-column root through root_product_kernel<true, .> -- t gathered in
    every block, one chunk, odd k (the pair loads reach the padding column)"""
    s, levels, roots = built_with_plan(pkg, monkeypatch, capfd, BINARY)
    assert any(R["fused"] and R["chunks"] == 1 and R["k"] % 2 == 1 and R["k"] > 1024 for R in roots), roots
    check_solves(s, *ref_nh)
    check_frames(pkg, BINARY, monkeypatch, frames_default)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", ["gpu", "host"])
@pytest.mark.parametrize("tree", ["default", "binary"])
def test_h_device_vs_host_factorization(pkg, monkeypatch, ref_nh, ref_edited, frames_default, tree, factor):
    """(h) the numeric factorization on the device (64-column Cholesky / inverse blocks, recursive doubling for L11^-1, the root's explicit
    inverse) and on the host (ADMM_HIP_FACTOR=host), on the trees of cases (a) and (e), against the reference; then again after
    set_weights + recompute_weights (anchors at half weight, every third tet at twice its weight) against the rebuilt reference"""
    env = dict(BINARY_SPLIT_TOP) if tree == "binary" else {}
    if factor == "host":
        env["ADMM_HIP_FACTOR"] = "host"
    set_env(monkeypatch, env)
    s = bar(pkg)
    assert s.info()["device_factor"] == (1 if factor == "gpu" else 0)
    check_solves(s, *ref_nh)
    nt = s.n_tets
    w = edited_weights(np.concatenate([s.read_rest(0)["weight"], s.read_rest(1)["weight"]]))
    assert np.array_equal(w, edited_weights(ref_nh[0].w0))      # the library's and the oracle's weights: bit for bit
    s.set_weights(0, w[:nt]); s.set_weights(1, w[nt:]); s.recompute_weights()
    check_solves(s, *ref_edited)
    if factor == "host" and tree == "default":
        check_frames(pkg, env, monkeypatch, frames_default)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"ADMM_HIP_ROOT_INVERSE": "0"}], ids=["default", "root_inverse_0"])
def test_i_stiff_badly_conditioned(pkg, monkeypatch, ref_stiff, ref_nh, env):
    """(i) mu = lam = 1e7 at density 100 with the upper half's weights at 1e-3 (stiffness contrast 1e6; stiff_weights):
    kappa1 >= 100x the default bar's (~7e6 against 1.6e4); forward error within fwd_tol(kappa1).  The contrast is bad scaling, which
    Cholesky does not feel: equilibrated, the matrix has kappa1_eq = 6.4e3, and the forward error is also held to
    EQ_C * 2^-53 * kappa1_eq = 2.9e-12, a hundred times below fwd_tol(kappa1) (measured: 0.24 x 2^-53 kappa1_eq on the host path, 0.245 on the MI355X:
    test_host_path_stiff_meets_the_kappa_rule; tests/test_ill_conditioned.py climbs where kappa1_eq itself is large)"""
    ref = ref_stiff[0]
    assert ref.kappa1 >= 100 * ref_nh[0].kappa1
    set_env(monkeypatch, env)
    s = stiff_bar(pkg)
    errs = check_solves(s, *ref_stiff)
    print("equilibrated kappa1 %.3g: forward errors %s x 2^-53 kappa1_eq (bound %g)" % (ref.kappa1_eq, ", ".join("%.3g" % (e / (EQ_EPS * ref.kappa1_eq)) for e in errs), EQ_C))
    assert max(errs) <= EQ_C * EQ_EPS * ref.kappa1_eq, (errs, ref.kappa1_eq)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 8])
def test_j_distributed_top(pkg, monkeypatch, capfd, ref_nh, world):
    """(j) ADMM_HIP_DIST_TOP=1, subtree shards, `world` ranks as threads of this process on one GPU: every rank factors its subtrees and its
    rows of the root (koff row slices) and runs root_product_kernel over its rows only (nrows < k); every rank's x against the reference,
    all ranks bitwise equal.  The distributed root holds the separators of the first max(2, log2 world) bisection levels: at 2 and 4 ranks
    three cross-sections (1 953 columns, one chunk), at 8 ranks seven separators (more than 2 048 columns: the row slices in two chunks)."""
    from test_sharding import _thread_allreduce_hooks
    monkeypatch.setenv("ADMM_HIP_DIST_TOP", "1")
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    capfd.readouterr()
    shards = [pkg.make_bar_system(*DIMS, device_id=0, rank=r, world=world, shard_mode="subtree") for r in range(world)]
    hooks = _thread_allreduce_hooks(world)
    for r, s in enumerate(shards):
        s.set_allreduce(hooks[r])
    pkg.initialize_together(shards)
    _, _, dist = plan(capfd.readouterr().err)
    assert len(dist) == world and all(0 < d["nrows"] < d["k"] for d in dist), dist
    if world == 8:
        assert all(d["chunks"] == 2 for d in dist), dist
    assert sorted((d["r0"], d["r1"]) for d in dist)[0][0] == 0 and sum(d["nrows"] for d in dist) == dist[0]["k"]
    assert all(s.info()["dist_top"] == 1 for s in shards)
    ref, x, m3 = ref_nh
    tol = fwd_tol(ref.kappa1)
    for i, b in enumerate(checkers.solve_rhs(7, x, m3)):
        out, errs = [None] * world, []

        def run(r):
            try:
                out[r] = shards[r].solve_only(b)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]; [t.join(timeout=300) for t in th]
        assert not errs and all(o is not None for o in out), errs
        xr, _, _ = ref.solve(b)
        for r in range(world):
            assert np.array_equal(out[r], out[0]), (i, r)
            err = np.abs(out[r] - xr).max() / np.abs(xr).max()
            assert err <= tol, (i, r, err)
        assert ref.backward_error(out[0], b) <= BWD_ERR_TOL


DENSE_CASES = [((7, 7, 31), None, 1), ((7, 7, 31), "2047", 0), ((2, 2, 3), None, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dims,dense_max,dense", DENSE_CASES, ids=["2048_nodes_dense", "2048_nodes_sparse", "36_nodes_dense"])
def test_k_dense_path_boundaries(pkg, monkeypatch, dims, dense_max, dense):
    """(k) the 7x7x31 bar (exactly 2 048 nodes) on the explicit inverse (dense_solve_kernel) and, with ADMM_HIP_DENSE_MAX=2047, on the
    sparse path; a 36-node bar, where dense_solve_kernel runs its tail loop only"""
    if dense_max:
        monkeypatch.setenv("ADMM_HIP_DENSE_MAX", dense_max)
    ref, x, m3 = checkers.bar_reference(pkg.meshgen, dims)
    s = pkg.make_bar_system(*dims, device_id=0)
    s.initialize()
    assert s.info()["n_nodes"] == x.shape[0] and s.info()["dense_solve"] == dense
    check_solves(s, ref, x, m3, host_sweeps=not dense)
