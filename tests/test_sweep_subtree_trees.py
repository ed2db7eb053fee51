"""The fused forward sweep over the bottom subtrees (sweep_plan.hpp plan_fused_subtrees, solve_fwd_subtree_kernel) on elimination-tree shapes
the structured bars of tests/test_sweep_subtree.py never give it: front rows fed by three or four children, children several levels
below their parent, subtrees of different depths in one launch, members without contribution rows (a forest of disconnected
bodies), eight-way trees, a narrow kernel cap, and irregular subtree shards.

Every case first asserts from the sweep plan (ADMM_HIP_VERBOSE: one "plan fused" line per call of upload_factor, its fields below)
that it reached the shape it exists for -- a case that fuses nothing fails -- and then checks

  * bitwise: the three right-hand sides of checkers.solve_rhs solve to the same x, bit for bit, as the per-level path
    (ADMM_HIP_SWEEP_FUSE=0, whose own plan line must say so); after two frames of ten iterations (corotational or StVK tets) m_x
    and m_v are bitwise equal too;
  * against the extended-precision reference (checkers.SparseReference, built through the oracle): test_wide_supernodes.check_solves
    -- forward error within fwd_tol(kappa1), normwise backward error 1e-14, host sweeps over the device's panels 1e-12 -- so that a
    bug shared by the fused and the per-level path is caught as well.

Plan fields: cut level, fused subtrees, subtrees left on the per-level path, LDS bytes of the largest record, the LDS cap, the
smallest..largest number of levels in one record, maxin (the most child contributions into one front row of a fused record),
skip (fused members whose parent lies two or more levels up), empty (non-root fused members with no contribution rows).  The
plans in the docstrings are those seen on one MI355X (256 CUs: a cut needs at least 512 subtrees).

Sensitivity, checked once with deliberately broken kernels: without the ab_c.z / ab_c.w adds case a fails its first solve; with the
first level of every record skipped cases b and c fail theirs.
"""
import re
import threading

import numpy as np
import pytest

import checkers
from test_wide_supernodes import BWD_ERR_TOL, RES_TOL, check_solves, fwd_tol, ref_nh, set_env  # noqa: F401 (ref_nh: fixture)

DIMS = (24, 24, 60)
DELAUNAY_PTS = 40000
LEAF8 = {"ADMM_HIP_LEAF": "8"}
FOUR_WAY = {"ADMM_HIP_LEAF": "16", "ADMM_HIP_MERGE": "10"}       # case a: four-way nodes down to regions of 10 nodes
CUT_A = 1                                                        # case a's cut level (its plan below)
FUSED = re.compile(r"admm_hip: plan fused (?:off \(([^)]*)\)|cut (\d+) subtrees (\d+) left (\d+) lds (\d+) cap (\d+) levels (\d+)\.\.(\d+) "
                   r"maxin (\d+) skip (\d+) empty (\d+))")
KEYS = ("cut", "subtrees", "left", "lds", "cap", "lv_min", "lv_max", "maxin", "skip", "empty")


def fused_plans(err):
    """the "plan fused" lines of admm_hip's stderr -> [{"off": reason} or {cut, subtrees, ..., empty}]"""
    out = []
    for m in FUSED.finditer(err):
        out.append({"off": m.group(1)} if m.group(1) is not None else dict(zip(KEYS, map(int, m.groups()[1:]))))
    return out


# ---------------------------------------------------------------- scenes and references (once per module) ----
@pytest.fixture(scope="module")
def delaunay():
    return checkers.delaunay_scene(DELAUNAY_PTS)


@pytest.fixture(scope="module")
def forest(pkg):
    return checkers.forest_scene(pkg.meshgen)


@pytest.fixture(scope="module")
def ref_delaunay(delaunay):
    x, m3, forces = delaunay
    return checkers.scene_reference(x, m3, forces), x, m3


@pytest.fixture(scope="module")
def ref_forest(forest):
    x, m3, forces = forest
    return checkers.scene_reference(x, m3, forces), x, m3


def stvk_bar(pkg):
    """the 24x24x60 bar of test_wide_supernodes with StVK tets (a deterministic frame): the same weights and selector rows as its
    Neo-Hookean reference, hence the same A"""
    return pkg.make_bar_system(*DIMS, kind=pkg.KIND["TET_STVK"])


# ---------------------------------------------------------------- helpers ----
def pair(monkeypatch, capfd, env, make):
    """(per-level system, fused system, the fused one's plan), both initialized under `env`"""
    set_env(monkeypatch, env)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    out, plans = [], []
    for fuse in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE", fuse)
        capfd.readouterr()
        s = make()
        s.initialize()
        out.append(s)
        plans.append(fused_plans(capfd.readouterr().err))
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    assert plans[0] == [{"off": "ADMM_HIP_SWEEP_FUSE=0"}], plans[0]
    assert len(plans[1]) == 1, plans[1]
    print("plan:", plans[1][0])
    return out[0], out[1], plans[1][0]


def check_bitwise_and_reference(per_level, fused, ref, x, m3):
    for i, b in enumerate(checkers.solve_rhs(7, x, m3)):
        assert np.array_equal(per_level.solve_only(b), fused.solve_only(b)), ("solve", i)
    check_solves(fused, ref, x, m3)
    for f in range(2):
        per_level.step(10); fused.step(10)
        assert np.array_equal(per_level.m_x, fused.m_x), ("frame", f)
        assert np.array_equal(per_level.m_v, fused.m_v), ("frame", f)


def same_weights(s, ref):
    w = np.concatenate([s.read_rest(0)["weight"], s.read_rest(1)["weight"]])
    assert np.array_equal(w, ref.w0), "the system's weights are not its reference's"


# ---------------------------------------------------------------- CPU: the host path on the irregular scenes ----
@pytest.mark.parametrize("scene", ["delaunay", "forest"])
def test_host_path_meets_the_bounds_on_irregular_trees(pkg, monkeypatch, request, scene):
    """the library's host path (host factorization, debug_panel_solve_host) on the scenes of cases b and c with their knobs, against
    the reference at the GPU cases' bounds: the calibration of those bounds on hardware-independent arithmetic"""
    set_env(monkeypatch, LEAF8)
    x, m3, forces = request.getfixturevalue(scene)
    ref = request.getfixturevalue("ref_" + scene)[0]
    s = checkers.scene_system(pkg, x, m3, forces, device_id=-1)
    s.initialize()
    tol = fwd_tol(ref.kappa1)
    for i, b in enumerate(checkers.solve_rhs(7, x, m3)):
        xr, _, _ = ref.solve(b)
        xs = s.debug_panel_solve_host(b)
        err = np.abs(xs - xr).max() / np.abs(xr).max()
        eta = ref.backward_error(xs, b)
        print("host path (%s, kappa1 %.3g): forward %.2g (tol %.2g), backward error %.2g" % (scene, ref.kappa1, err, tol, eta))
        assert err <= tol and eta <= BWD_ERR_TOL, (i, err, eta)
        if i == 0:
            assert np.abs(ref.residual(xs, b)).max() <= RES_TOL * np.abs(b).max()


def test_scenes_have_the_intended_structure(delaunay, forest):
    """the Delaunay mesh is irregular (node valence spread) and the forest is hundreds of connected components"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    x, _, forces = delaunay
    t = forces[0][1]
    deg = np.bincount(t.ravel(), minlength=x.shape[0])
    assert x.shape[0] == DELAUNAY_PTS and deg.max() > 2 * deg.mean() and deg.min() < 0.5 * deg.mean(), (deg.min(), deg.mean(), deg.max())
    x, _, forces = forest
    t = forces[0][1]
    e = np.concatenate([t[:, [a, b]] for a in range(4) for b in range(a + 1, 4)])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(x.shape[0],) * 2)
    n, lab = connected_components(g, directed=False)
    sizes = np.bincount(lab)
    assert n > 300 and sizes.max() > 10 * np.median(sizes), (n, sizes.max())


# ---------------------------------------------------------------- GPU ----
@pytest.mark.gpu
def test_a_four_way_subtrees(pkg, monkeypatch, capfd, ref_nh):
    """(a) the 24x24x60 bar with ADMM_HIP_LEAF=16 MERGE=10: four-way nodes inside the fused subtrees, front rows fed by all four
    children (ab_c.z / ab_c.w and ab_t.z / ab_t.w of the kernel).  Plan: cut 1, 787 subtrees, left 0, levels 1..2, maxin 4,
    skip 0, empty 0"""
    ref, x, m3 = ref_nh
    per_level, fused, plan = pair(monkeypatch, capfd, FOUR_WAY, lambda: stvk_bar(pkg))
    assert plan.get("cut") == CUT_A and plan["subtrees"] >= 512 and plan["maxin"] == 4 and plan["lv_max"] >= 2, plan
    same_weights(fused, ref)
    check_bitwise_and_reference(per_level, fused, ref, x, m3)


@pytest.mark.gpu
def test_b_unbalanced_irregular_subtrees(pkg, monkeypatch, capfd, delaunay, ref_delaunay):
    """(b) the 40 000-point Delaunay mesh with ADMM_HIP_LEAF=8: children several levels below their parent and subtrees of different
    depths in one launch.  Plan: cut 2, 774 subtrees, left 0, levels 1..3, maxin 2, skip 464, empty 0"""
    per_level, fused, plan = pair(monkeypatch, capfd, LEAF8, lambda: checkers.scene_system(pkg, *delaunay))
    assert plan.get("subtrees", 0) >= 512 and plan["skip"] > 0 and plan["lv_min"] < plan["lv_max"], plan
    check_bitwise_and_reference(per_level, fused, *ref_delaunay)


@pytest.mark.gpu
def test_c_forest_with_empty_members(pkg, monkeypatch, capfd, forest, ref_forest):
    """(c) a few hundred small bodies beside one larger bar, ADMM_HIP_LEAF=8: dissection regions that split between bodies give
    supernodes without contribution rows under a parent.  Plan: cut 2, 623 subtrees, left 0, levels 1..3, maxin 2, skip 279, empty 4"""
    per_level, fused, plan = pair(monkeypatch, capfd, LEAF8, lambda: checkers.scene_system(pkg, *forest))
    assert plan.get("subtrees", 0) >= 512 and plan["empty"] > 0, plan
    check_bitwise_and_reference(per_level, fused, *ref_forest)


@pytest.mark.gpu
def test_d_eight_way_tree(pkg, monkeypatch, capfd, ref_nh):
    """(d) case a with ADMM_HIP_MERGE_DEPTH=3: eight-way nodes.  No front row of this tree gets more than four contributions, so it
    still fuses (fusion is not off for want of cg4).  Plan: cut 1, 512 subtrees, left 0, levels 1..2, maxin 3, skip 0, empty 0"""
    ref, x, m3 = ref_nh
    per_level, fused, plan = pair(monkeypatch, capfd, dict(FOUR_WAY, ADMM_HIP_MERGE_DEPTH="3"), lambda: stvk_bar(pkg))
    assert plan.get("subtrees", 0) >= 512 and plan["maxin"] == 3, plan
    check_bitwise_and_reference(per_level, fused, ref, x, m3)


@pytest.mark.gpu
def test_e_narrow_kernel_cap(pkg, monkeypatch, capfd, ref_nh):
    """(e) case a with ADMM_HIP_FWD_SMALL_K=16: only supernodes of at most 16 columns may be fused, so the cut drops below case a's.
    Plan: cut 0, 1199 subtrees, left 0, levels 1..1, maxin 0, skip 0, empty 0"""
    ref, x, m3 = ref_nh
    per_level, fused, plan = pair(monkeypatch, capfd, dict(FOUR_WAY, ADMM_HIP_FWD_SMALL_K="16"), lambda: stvk_bar(pkg))
    assert plan.get("off") == "no cut level" or plan["cut"] < CUT_A, plan
    check_bitwise_and_reference(per_level, fused, ref, x, m3)


@pytest.mark.gpu
def test_f_irregular_subtree_shards(pkg, monkeypatch, capfd, delaunay, ref_delaunay):
    """(f) case b's scene and knobs as two subtree shards on one GPU (threads + an in-process all-reduce): every rank fuses its own
    bottom subtrees; solves and two frames are bitwise equal between the ranks and between the fused and the per-level runs, and the
    solves match the unsharded run to 1e-10.  Plans of the two ranks: cut 1, 520 and 524 subtrees (left 0, levels 1..2, maxin 3,
    skip 0, empty 0 on both)"""
    from test_sharding import _thread_allreduce_hooks
    ref, x, m3 = ref_delaunay
    B = checkers.solve_rhs(7, x, m3)
    set_env(monkeypatch, LEAF8)
    whole = checkers.scene_system(pkg, *delaunay)
    whole.initialize()
    x_whole = [whole.solve_only(b) for b in B]
    del whole
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    runs = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE", fuse)
        capfd.readouterr()
        shards = [checkers.scene_system(pkg, *delaunay, rank=r, world=2) for r in range(2)]
        hooks = _thread_allreduce_hooks(2)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(shards)
        plans = fused_plans(capfd.readouterr().err)
        print("plans (fuse %s):" % fuse, plans)
        if fuse == "1":
            assert len(plans) == 2 and all(p.get("subtrees", 0) > 0 for p in plans), plans
        else:
            assert plans == [{"off": "ADMM_HIP_SWEEP_FUSE=0"}] * 2, plans
        errs = []

        def on_ranks(fn):
            out = [None] * 2

            def run(r):
                try:
                    out[r] = fn(shards[r])
                except BaseException as e:  # noqa: BLE001 (surface failures of a worker thread)
                    errs.append(e)
            th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
            [t.start() for t in th]; [t.join(timeout=300) for t in th]
            assert not errs and all(o is not None for o in out), errs
            assert all(np.array_equal(o, out[0]) for o in out), fuse      # ranks bitwise equal
            return out[0]
        sols = [on_ranks(lambda s: s.solve_only(b)) for b in B]

        def frame(s):
            s.step(10); s.sync()
            return np.concatenate([s.m_x, s.m_v])
        frames = [on_ranks(frame) for _ in range(2)]
        runs[fuse] = sols + frames
        del shards
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    for i, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert np.array_equal(a, b), ("fused vs per-level", i)
    tol = fwd_tol(ref.kappa1)
    for i, b in enumerate(B):
        xs = runs["1"][i]
        assert np.abs(xs - x_whole[i]).max() <= 1e-10 * np.abs(x_whole[i]).max(), ("sharded vs unsharded", i)
        xr, _, _ = ref.solve(b)
        assert np.abs(xs - xr).max() <= tol * np.abs(xr).max(), ("forward error", i)
        assert ref.backward_error(xs, b) <= BWD_ERR_TOL, ("backward error", i)
