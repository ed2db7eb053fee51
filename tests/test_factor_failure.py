"""A system matrix that is not positive definite is refused, on every factorization path and by every rank.

Ground truth: one chosen node i gets a negative mass with m_i + (dt^2 D^T W^2 D)_ii < 0, the second term taken from the ORACLE's
selector D and weight diagonal (the assembly checkers.SparseReference factors).  A symmetric matrix with a negative diagonal entry is
not positive definite, and every Schur complement of that entry is <= the entry itself, while the leading principal submatrix in front
of it is that of a positive definite matrix: the first pivot that is not positive is node i's own, in the supernode whose columns hold
it.  So the expected outcome is exact: ADMM_ERR_FACTOR naming that supernode (admm_hip_debug_node_supernode), on the device
factorization and on the host one (ADMM_HIP_FACTOR=host, host-only contexts) alike.  The second corruption is a NaN weight
(set_weights + recompute_weights): refused everywhere, naming the lowest-numbered supernode that holds one of the tet's nodes.

Paths: a leaf, an interior supernode of a four-way merged tree, the merged root with its explicit inverse, a root factored through
the sweeps, a supernode wider than 64 columns with the failing pivot in its second 64-column block, the dense small-system path.
Each case first asserts, on a healthy twin, that it reaches the path it exists for.  After a failed recompute_weights the context
refuses step / solve_only / local_step_* (ADMM_ERR_STATE) until a recompute_weights succeeds, after which its solves are those of a
twin that never failed, bit for bit.

Shards (N contexts in one process on one GPU, thread hooks whose barrier times out instead of hanging): every rank raises
ADMM_ERR_FACTOR naming the same supernode, on initialize and on recompute_weights -- rank-local factorization with the replicated
and the distributed top, every rank factoring the whole matrix, contiguous shards.
"""
import functools
import re
import threading

import numpy as np
import pytest

import checkers

DT = 0.04
ERR_STATE, ERR_FACTOR = 3, 5
BARRIER_TIMEOUT = 120.0


# ---------------------------------------------------------------- scenes ----
def bar_arrays(pkg, dims):
    x, t = pkg.meshgen.bar(*dims)
    return x, t, pkg.meshgen.lumped_tet_mass(x, t, 1000.0), pkg.meshgen.bar_anchor_nodes(dims[0], dims[1])


@functools.lru_cache(maxsize=None)
def _stiffness_diag(dims):
    from __graft_entry__ import load_package
    x, t, m, anchors = bar_arrays(load_package(), dims)
    o = checkers.Oracle(); o.settings(DT, 1)
    o.add_nodes(x.ravel(), np.repeat(m, 3))
    o.add_forces(checkers.KIND["TET_NH"], t, [1e5, 1e5, 5])
    o.add_forces(checkers.KIND["ANCHOR"], anchors, [-1.0, 1.0])
    assert o.initialize()
    rr, cc, vv = o.D_triplets()
    W = o.wdiag
    k = np.bincount(cc, weights=(DT * DT) * (W[rr] ** 2) * vv * vv, minlength=3 * x.shape[0])      # diag(dt^2 D^T W^2 D), per dof
    assert np.array_equal(k[0::3], k[1::3]) and np.array_equal(k[0::3], k[2::3])
    return k[0::3]


def negative_mass(pkg, dims, i):
    """the bar's masses with node i's made so negative that A_ii = m_i + (dt^2 D^T W^2 D)_ii < 0"""
    _, _, m, _ = bar_arrays(pkg, dims)
    k = _stiffness_diag(tuple(dims))
    m = m.copy()
    m[i] = -(2.0 * k[i] + m[i])
    assert m[i] + k[i] < 0.0
    return m


def bar(pkg, dims, masses=None, device_id=0, rank=0, world=1, shard_mode=None):
    """make_bar_system's bar, with other masses if given"""
    x, t, m, anchors = bar_arrays(pkg, dims)
    s = pkg.System(device_id=device_id)
    s.set_timestep(DT)
    s.add_nodes(x.ravel(), np.repeat(m if masses is None else masses, 3))
    s.add_forces(pkg.KIND["TET_NH"], t, [1e5, 1e5, 5])
    s.add_forces(pkg.KIND["ANCHOR"], anchors, [-1.0, 1.0])
    s.add_gravity((0.0, -9.8, 0.0))
    if world > 1:
        s.set_shard(rank, world)
        if shard_mode is not None:
            s.set_shard_mode(shard_mode)
    s.n_tets = t.shape[0]
    return s


def named_supernode(err):
    m = re.search(r"not positive definite \(supernode (\d+)\)", str(err))
    assert m, "no supernode named: %s" % err
    return int(m.group(1))


def refused(pkg, call):
    """call() must raise AdmmHipError for a matrix that is not positive definite -> the supernode it names"""
    with pytest.raises(pkg.AdmmHipError) as e:
        call()
    assert "admm_hip error %d" % ERR_FACTOR in str(e.value), str(e.value)
    return named_supernode(e.value)


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def plan_roots(err):
    """root lines of the sweep plan (upload.inc, ADMM_HIP_VERBOSE): explicit-inverse roots"""
    return re.findall(r"admm_hip: plan (?:own|top) level \d+: root k (\d+) (?:fused|gather)", err)


# ---------------------------------------------------------------- single-context cases ----
def _leaf(sn, col, par):
    kids = np.bincount(par[par >= 0], minlength=par.size)
    return [s for s in range(par.size) if kids[s] == 0 and par[s] >= 0]


def _four_way_interior(sn, col, par):
    kids = np.bincount(par[par >= 0], minlength=par.size)
    return [s for s in range(par.size) if kids[s] == 4 and par[s] >= 0]


def _root(sn, col, par):
    return [s for s in range(par.size) if par[s] < 0]


def _wide(sn, col, par):
    """supernodes of more than 64 columns, not roots first"""
    wide = sorted(set(sn[col >= 64].tolist()), key=lambda s: (par[s] < 0, s))
    return wide


BASE = {"ADMM_HIP_DENSE_MAX": "0"}
CASES = {
    # name: (bar, env, supernode selector, the node's column inside it must be >= this)
    "leaf": ((6, 6, 16), dict(BASE), _leaf, 0),
    "four_way_interior": ((8, 8, 40), dict(BASE, ADMM_HIP_MERGE="100"), _four_way_interior, 0),
    "merged_root_inverse": ((6, 6, 20), dict(BASE, ADMM_HIP_TREE_SEARCH="0", ADMM_HIP_MERGE="0"), _root, 0),
    "root_by_sweeps": ((6, 6, 20), dict(BASE, ADMM_HIP_TREE_SEARCH="0", ADMM_HIP_MERGE="0", ADMM_HIP_MERGE_ROOT="0",
                                        ADMM_HIP_ROOT_INVERSE="0"), _root, 0),
    "wide_second_block": ((10, 10, 30), dict(BASE), _wide, 64),
}


def pick_node(s, select, min_col):
    """-> (node, its supernode): a node of the first supernode `select` gives, at the column min_col + a third of the rest"""
    sn, col, par = s.node_supernode()
    cands = select(sn, col, par)
    assert cands, "the tree has no supernode of this kind"
    target = cands[0]
    nodes = np.flatnonzero(sn == target)
    ncols = nodes.size
    assert ncols > min_col, (target, ncols)
    want = min_col + (ncols - min_col) // 3
    i = int(nodes[np.flatnonzero(col[nodes] == want)[0]])
    return i, target, par


def check_path(name, s, target, par, err, device):
    inf = s.info()
    assert inf["dense_solve"] == 0
    if device:
        assert inf["device_factor"] == 1
    if name == "merged_root_inverse":
        assert par[target] < 0
        if device:
            assert plan_roots(err), "no explicit-inverse root in the sweep plan"
    if name == "root_by_sweeps":
        assert par[target] < 0
        if device:
            assert not plan_roots(err), "the root was not left to the sweeps"


def run_single(pkg, monkeypatch, capfd, name, device_id):
    dims, env, select, min_col = CASES[name]
    set_env(monkeypatch, env)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    capfd.readouterr()
    twin = bar(pkg, dims, device_id=device_id)
    twin.initialize()
    err = capfd.readouterr().err
    i, target, par = pick_node(twin, select, min_col)
    check_path(name, twin, target, par, err, device_id >= 0)
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    got = refused(pkg, bar(pkg, dims, negative_mass(pkg, dims, i), device_id=device_id).initialize)
    assert got == target, (name, "node", i, "named", got, "expected", target)
    return i, target


@pytest.mark.parametrize("name", list(CASES))
def test_host_factorization_names_the_supernode(pkg, monkeypatch, capfd, name):
    """host-only contexts (host_assemble + host_factor): refused, naming the node's own supernode"""
    run_single(pkg, monkeypatch, capfd, name, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_factorization_names_the_supernode(pkg, monkeypatch, capfd, name):
    """device factorization: refused, naming the node's own supernode -- and the host factorization of the same system names it too"""
    i, target = run_single(pkg, monkeypatch, capfd, name, 0)
    dims = CASES[name][0]
    monkeypatch.setenv("ADMM_HIP_FACTOR", "host")
    got = refused(pkg, bar(pkg, dims, negative_mass(pkg, dims, i), device_id=0).initialize)
    assert got == target, (name, "host factorization named", got, "device", target)


# ---------------------------------------------------------------- dense small-system path ----
DENSE_DIMS = (4, 4, 12)


@pytest.mark.parametrize("device_id", [-1, pytest.param(0, marks=pytest.mark.gpu)])
def test_dense_path_refused(pkg, device_id):
    """<= 2048 nodes (default ADMM_HIP_DENSE_MAX): refused before A^-1 is formed"""
    twin = bar(pkg, DENSE_DIMS, device_id=device_id)
    twin.initialize()
    assert twin.info()["dense_solve"] == 1
    sn, _, _ = twin.node_supernode()
    i = int(np.argmax(bar_arrays(pkg, DENSE_DIMS)[0][:, 2]))      # a node at the free end
    s = bar(pkg, DENSE_DIMS, negative_mass(pkg, DENSE_DIMS, i), device_id=device_id)
    assert refused(pkg, s.initialize) == sn[i]
    assert s.info()["dense_solve"] == 0
    with pytest.raises(pkg.AdmmHipError):
        s.step(1)


# ---------------------------------------------------------------- NaN weights, recompute_weights ----
def nan_weights(s, tet):
    w = s.read_rest(0)["weight"].copy()
    w[tet] = np.nan
    return w


def nan_expected(pkg, s, dims, tet):
    sn, _, _ = s.node_supernode()
    return int(sn[bar_arrays(pkg, dims)[1][tet]].min())


RECOMPUTE_DIMS, RECOMPUTE_ENV = (6, 6, 20), {"ADMM_HIP_DENSE_MAX": "0"}


@pytest.mark.parametrize("dense", [False, True])
def test_host_recompute_nan_weight_refused(pkg, monkeypatch, dense):
    if not dense:
        set_env(monkeypatch, RECOMPUTE_ENV)
    dims = RECOMPUTE_DIMS if not dense else DENSE_DIMS
    s = bar(pkg, dims, device_id=-1)
    s.initialize()
    tet = s.n_tets // 2
    w0 = s.read_rest(0)["weight"].copy()
    s.set_weights(0, nan_weights(s, tet))
    assert refused(pkg, s.recompute_weights) == nan_expected(pkg, s, dims, tet)
    s.set_weights(0, w0)
    s.recompute_weights()


def assert_state_refusal(pkg, s, x):
    for what, call in (("step", lambda: s.step(2)), ("solve_only", lambda: s.solve_only(x)), ("local_step_only", lambda: s.local_step_only(x)),
                       ("local_step_dx", lambda: s.local_step_dx(0, np.zeros((s.n_tets, 9))))):
        with pytest.raises(pkg.AdmmHipError) as e:
            call()
        msg = str(e.value)
        assert "admm_hip error %d" % ERR_STATE in msg and "recompute_weights failed" in msg and "not positive definite" in msg, (what, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True])
def test_failed_recompute_refuses_until_restored(pkg, monkeypatch, dense):
    """after a recompute_weights that fails, step / solve_only / local_step_* refuse with ADMM_ERR_STATE; restoring the weights and
    recomputing makes the context usable again, its solves and frames bitwise those of a twin that never failed.  (Weights cannot make
    A_s indefinite -- they enter squared -- so a NaN weight is the failure a recompute can meet.)"""
    if not dense:
        set_env(monkeypatch, RECOMPUTE_ENV)
    dims = DENSE_DIMS if dense else RECOMPUTE_DIMS
    s, twin = bar(pkg, dims), bar(pkg, dims)
    s.initialize(); twin.initialize()
    assert s.info()["dense_solve"] == int(dense) and s.info()["device_factor"] == int(not dense)
    x0 = s.m_x.copy()
    b = np.random.default_rng(5).normal(size=x0.size)
    w0 = s.read_rest(0)["weight"].copy()
    tet = s.n_tets // 2
    s.set_weights(0, nan_weights(s, tet))
    expected = nan_expected(pkg, s, dims, tet)
    assert refused(pkg, s.recompute_weights) == expected
    assert_state_refusal(pkg, s, x0)
    s.set_weights(0, w0)
    s.recompute_weights()
    assert np.array_equal(s.solve_only(b), twin.solve_only(b))
    s.m_x = x0; twin.m_x = x0
    for _ in range(2):
        s.step(5); twin.step(5)
    assert np.array_equal(s.m_x, twin.m_x) and np.array_equal(s.m_v, twin.m_v)


# ---------------------------------------------------------------- shards: N contexts, one process, one GPU ----
def thread_allreduce_hooks(world):
    """tests/test_sharding.py's all-reduce between contexts of one process, with a barrier that times out: a rank left waiting
    makes its call fail (the hook returns 1 -> ADMM_ERR_COMM) instead of hanging the test"""
    import torch
    bar_ = threading.Barrier(world, timeout=BARRIER_TIMEOUT)
    bufs = {}

    class _Ptr:
        def __init__(self, ptr, count):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}

    def make_hook(r):
        def hook(ptr, count, stream):
            try:
                torch.cuda.synchronize()
                bufs[r] = torch.as_tensor(_Ptr(ptr, count), device="cuda:0")
                bar_.wait()
                if r == 0:
                    tot = bufs[0].clone()
                    for q in range(1, world):
                        tot += bufs[q]
                    for q in range(world):
                        bufs[q].copy_(tot)
                    torch.cuda.synchronize()
                bar_.wait()
                return 0
            except threading.BrokenBarrierError:
                bar_.abort()
                return 1
        return hook
    return [make_hook(r) for r in range(world)]


SHARD_DIMS = (6, 6, 48)
SHARD_ENV = {"ADMM_HIP_DENSE_MAX": "0", "ADMM_HIP_LEAF": "16"}
SHARD_CASES = {
    # name: (world, shard mode, factor_local, ADMM_HIP_DIST_TOP)
    "subtree2_replicated": (2, "subtree", True, "0"),
    "subtree4_replicated": (4, "subtree", True, "0"),
    "subtree2_dist_top": (2, "subtree", True, "1"),
    "subtree4_dist_top": (4, "subtree", True, "1"),
    "subtree2_not_local": (2, "subtree", False, "0"),
    "contiguous2": (2, "contiguous", True, "0"),
}


def shards(pkg, world, mode, local, masses=None):
    ss = [bar(pkg, SHARD_DIMS, masses, rank=r, world=world, shard_mode=mode) for r in range(world)]
    for s, h in zip(ss, thread_allreduce_hooks(world)):
        s.set_allreduce(h)
        if not local:
            s.set_factor_local(False)
    return ss


def all_refused(pkg, ss, call):
    """the collective call on every rank: each must raise ADMM_ERR_FACTOR, all naming the same supernode -> that supernode"""
    with pytest.raises(pkg.RankErrors) as e:
        pkg.call_together(ss, call, timeout=600.0, grace=BARRIER_TIMEOUT + 30.0)
    errs = e.value.errors
    assert all(isinstance(x, pkg.AdmmHipError) and "admm_hip error %d" % ERR_FACTOR in str(x) for x in errs), str(e.value)
    named = [named_supernode(x) for x in errs]
    assert len(set(named)) == 1, ("ranks name different supernodes", named)
    return named[0]


def healthy(pkg, monkeypatch, name):
    """the case's shards, initialized, after asserting they took the path the case exists for"""
    world, mode, local, dist = SHARD_CASES[name]
    set_env(monkeypatch, dict(SHARD_ENV, ADMM_HIP_DIST_TOP=dist))
    ss = shards(pkg, world, mode, local)
    pkg.call_together(ss, "initialize", timeout=600.0)
    inf = [s.info() for s in ss]
    assert all(f["world"] == world and f["dense_solve"] == 0 and f["device_factor"] == 1 for f in inf)
    assert all(f["factor_local"] == int(local and mode == "subtree") for f in inf), inf
    assert all(f["dist_top"] == int(dist == "1" and local and mode == "subtree") for f in inf), inf
    return ss


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["rank1", "top"])
@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_shards_initialize_all_refuse(pkg, monkeypatch, name, where):
    """a node owned by rank 1 alone, or one of the replicated top, made indefinite: every rank's initialize raises ADMM_ERR_FACTOR
    naming the node's supernode"""
    world, mode, local, _ = SHARD_CASES[name]
    ss = healthy(pkg, monkeypatch, name)
    sn, _, _ = ss[0].node_supernode()
    owner = ss[0].node_owner() if mode == "subtree" else None
    if owner is not None:
        cand = np.flatnonzero(owner == (1 if where == "rank1" else -1))
    else:       # contiguous shards: no owners, every rank factors everything -- the first / last node
        cand = np.arange(ss[0].n_nodes)
    assert cand.size, (name, where)
    i = int(cand[cand.size // 2] if where == "rank1" else cand[-1])
    got = all_refused(pkg, shards(pkg, world, mode, local, negative_mass(pkg, SHARD_DIMS, i)), "initialize")
    assert got == sn[i], (name, where, "node", i, "named", got, "expected", int(sn[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_shards_recompute_all_refuse(pkg, monkeypatch, name):
    """a NaN weight on a tet of rank 1's subtrees: every rank's recompute_weights raises ADMM_ERR_FACTOR naming the same supernode,
    every rank's step then refuses, and restoring the weights makes all ranks recompute"""
    world, mode, local, _ = SHARD_CASES[name]
    ss = healthy(pkg, monkeypatch, name)
    tets = bar_arrays(pkg, SHARD_DIMS)[1]
    sn, _, _ = ss[0].node_supernode()
    if mode == "subtree":
        owner = ss[0].node_owner()
        tet = int(np.flatnonzero((owner[tets] == 1).all(axis=1))[0])
    else:
        tet = tets.shape[0] // 2
    w0 = ss[0].read_rest(0)["weight"].copy()
    w = w0.copy(); w[tet] = np.nan
    for s in ss:
        s.set_weights(0, w)
    got = all_refused(pkg, ss, "recompute_weights")
    assert got == int(sn[tets[tet]].min()), (name, got, int(sn[tets[tet]].min()))
    for s in ss:
        with pytest.raises(pkg.AdmmHipError, match="admm_hip error %d" % ERR_STATE):
            s.step(1)
    for s in ss:
        s.set_weights(0, w0)
    pkg.call_together(ss, "recompute_weights", timeout=600.0)
