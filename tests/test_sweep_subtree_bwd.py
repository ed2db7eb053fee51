"""The fused backward sweep over the bottom subtrees (sweep_plan.hpp bwd_subtree_record, solve_bwd_kernel_subtree): the same x, BIT FOR
BIT, as the per-level backward launches under the same knobs (ADMM_HIP_SWEEP_FUSE_BWD=0: the forward sweep stays fused), on the scenes
of tests/test_sweep_subtree_trees.py.

Every GPU case first asserts from the sweep plan (ADMM_HIP_VERBOSE: one "plan fused_bwd" line per call of upload_factor) that backward
subtrees were fused at all and that the reference run fused none, so that a comparison of the per-level path with itself cannot
pass; then three right-hand sides of checkers.solve_rhs solve to the same x bit for bit, and m_x / m_v are bitwise equal after two
frames of ten iterations.

The CPU test covers the host check of a record (csrc/bwd_record.hpp bwd_record_check, through tests/bwd_record_shim.cpp) only: a
hand-written record passes; one out-of-range offset and, separately, one column written twice are refused.  The builder of the records is
exercised by the GPU cases: sweep_plan.hpp runs the same check on every record it builds and refuses to launch on a violation.
"""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import checkers
from test_sweep_subtree_trees import FOUR_WAY, LEAF8, delaunay, forest, fused_plans, stvk_bar  # noqa: F401 (fixtures)
from test_wide_supernodes import check_solves, ref_nh, set_env  # noqa: F401 (ref_nh: fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED_BWD = re.compile(r"admm_hip: plan fused_bwd (?:off \(([^)]*)\)|cut (\d+) subtrees (\d+) left (\d+) lds (\d+) cap (\d+))")
KEYS = ("cut", "subtrees", "left", "lds", "cap")
BWD_OFF = {"off": "ADMM_HIP_SWEEP_FUSE_BWD=0"}


def bwd_plans(err):
    """the "plan fused_bwd" lines of admm_hip's stderr -> [{"off": reason} or {cut, subtrees, left, lds, cap}]"""
    out = []
    for m in FUSED_BWD.finditer(err):
        out.append({"off": m.group(1)} if m.group(1) is not None else dict(zip(KEYS, map(int, m.groups()[1:]))))
    return out


def pair(monkeypatch, capfd, env, make):
    """(per-level backward system, fused backward system, the fused one's forward plan, its backward plan), both initialized under `env`
    with the forward sweep fused"""
    set_env(monkeypatch, env)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    out, fwd, bwd = [], [], []
    for on in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE_BWD", on)
        capfd.readouterr()
        s = make()
        s.initialize()
        out.append(s)
        err = capfd.readouterr().err
        fwd.append(fused_plans(err)); bwd.append(bwd_plans(err))
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    print("plans:", fwd, bwd)
    assert len(fwd[0]) == 1 and fwd[0] == fwd[1] and fwd[1][0].get("subtrees", 0) > 0, fwd      # the forward sweep: fused, and the same, in both
    assert bwd[0] == [BWD_OFF], bwd[0]
    assert len(bwd[1]) == 1 and bwd[1][0].get("subtrees", 0) > 0, bwd[1]
    assert bwd[1][0]["lds"] <= bwd[1][0]["cap"] and bwd[1][0]["cut"] == fwd[1][0]["cut"], (fwd[1], bwd[1])
    return out[0], out[1], fwd[1][0], bwd[1][0]


def check_bitwise(per_level, fused, x, m3):
    for i, b in enumerate(checkers.solve_rhs(7, x, m3)):
        assert np.array_equal(per_level.solve_only(b), fused.solve_only(b)), ("solve", i)
    for f in range(2):
        per_level.step(10); fused.step(10)
        assert np.array_equal(per_level.m_x, fused.m_x), ("frame", f)
        assert np.array_equal(per_level.m_v, fused.m_v), ("frame", f)


# ---------------------------------------------------------------- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("nw", [2, 4, 8, 16])
def test_1_lane_to_row_rule_for_every_block_width(pkg, monkeypatch, capfd, ref_nh, nw):
    """(1) the four-way 24x24x60 bar with ADMM_HIP_BWD_SMALL_NW = 2 / 4 / 8 / 16: a column's lanes start at the first row of its block of
    B = 8 / 16 / 32 / 64 columns.  Supernodes with k < B, with k no multiple of 4, fronts of fewer than 64 rows and of just over a
    multiple of 64 all occur among the fused members."""
    _, x, m3 = ref_nh
    per_level, fused, _, plan = pair(monkeypatch, capfd, dict(FOUR_WAY, ADMM_HIP_BWD_SMALL_NW=str(nw)), lambda: stvk_bar(pkg))
    assert plan["subtrees"] >= 512, plan
    check_bitwise(per_level, fused, x, m3)


@pytest.mark.gpu
def test_2_rows_in_members_several_levels_up(pkg, monkeypatch, capfd, delaunay):
    """(2) the 40 000-point Delaunay mesh with ADMM_HIP_LEAF=8: front rows of a member lie in members two or more levels up (skip > 0 in
    the forward plan: the same subtrees), and subtrees of different depths share the launch"""
    x, m3, _ = delaunay
    per_level, fused, fwd, plan = pair(monkeypatch, capfd, LEAF8, lambda: checkers.scene_system(pkg, *delaunay))
    assert plan["subtrees"] >= 512 and fwd["skip"] > 0 and fwd["lv_min"] < fwd["lv_max"], (fwd, plan)
    check_bitwise(per_level, fused, x, m3)


@pytest.mark.gpu
def test_3_forest_members_without_rows(pkg, monkeypatch, capfd, forest):
    """(3) the forest of small bodies beside one bar, ADMM_HIP_LEAF=8: members without front rows beyond their columns (empty > 0 in
    the forward plan) and members all of whose rows lie above the subtree"""
    x, m3, _ = forest
    per_level, fused, fwd, plan = pair(monkeypatch, capfd, LEAF8, lambda: checkers.scene_system(pkg, *forest))
    assert plan["subtrees"] >= 512 and fwd["empty"] > 0, (fwd, plan)
    check_bitwise(per_level, fused, x, m3)


@pytest.mark.gpu
def test_4_subtrees_left_on_the_per_level_path(pkg, monkeypatch, capfd):
    """(4) the 24x24x400 bar (four fused levels): some subtrees need more LDS than the cap and keep their per-level launches in one or
    both sweeps, next to the fused launches"""
    per_level, fused, fwd, plan = pair(monkeypatch, capfd, {}, lambda: pkg.make_bar_system(24, 24, 400))
    assert fwd["left"] > 0 or plan["left"] > 0, (fwd, plan)
    n = fused.info()["n_nodes"]
    rng = np.random.default_rng(7)
    for i in range(3):
        b = rng.standard_normal(3 * n)
        assert np.array_equal(per_level.solve_only(b), fused.solve_only(b)), ("solve", i)
    for f in range(2):
        per_level.step(10); fused.step(10)
        assert np.array_equal(per_level.m_x, fused.m_x), ("frame", f)
        assert np.array_equal(per_level.m_v, fused.m_v), ("frame", f)


@pytest.mark.gpu
def test_5_two_subtree_shards(pkg, monkeypatch, capfd, delaunay):
    """(5) case 2's scene as two subtree shards on one GPU (threads + an in-process all-reduce): every rank fuses its own subtrees in
    both sweeps; solves and two frames are bitwise equal between the ranks and to the run with per-level backward launches"""
    from test_sharding import _thread_allreduce_hooks
    x, m3, _ = delaunay
    B = checkers.solve_rhs(7, x, m3)
    set_env(monkeypatch, LEAF8)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    runs = {}
    for on in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE_BWD", on)
        capfd.readouterr()
        shards = [checkers.scene_system(pkg, *delaunay, rank=r, world=2) for r in range(2)]
        hooks = _thread_allreduce_hooks(2)
        for r, s in enumerate(shards):
            s.set_allreduce(hooks[r])
        pkg.initialize_together(shards)
        err = capfd.readouterr().err
        fwd, plans = fused_plans(err), bwd_plans(err)
        print("plans (bwd %s):" % on, fwd, plans)
        assert len(fwd) == 2 and all(p.get("subtrees", 0) > 0 for p in fwd), fwd
        if on == "1":
            assert len(plans) == 2 and all(p.get("subtrees", 0) > 0 for p in plans), plans
        else:
            assert plans == [BWD_OFF] * 2, plans
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
            assert all(np.array_equal(o, out[0]) for o in out), on      # ranks bitwise equal
            return out[0]
        sols = [on_ranks(lambda s: s.solve_only(b)) for b in B]

        def frame(s):
            s.step(10); s.sync()
            return np.concatenate([s.m_x, s.m_v])
        frames = [on_ranks(frame) for _ in range(2)]
        runs[on] = sols + frames
        del shards
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    for i, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert np.array_equal(a, b), ("fused vs per-level backward", i)


@pytest.mark.gpu
def test_6_against_the_extended_precision_reference(pkg, monkeypatch, capfd, ref_nh):
    """(6) case 1's system with the default block width, both sweeps fused, against the extended-precision reference
    (test_wide_supernodes.check_solves: forward error, backward error, host sweeps over the device's panels): a bug the fused and the
    per-level backward path share is caught here"""
    ref, x, m3 = ref_nh
    set_env(monkeypatch, FOUR_WAY)
    monkeypatch.setenv("ADMM_HIP_VERBOSE", "1")
    capfd.readouterr()
    s = stvk_bar(pkg)
    s.initialize()
    plans = bwd_plans(capfd.readouterr().err)
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    assert len(plans) == 1 and plans[0].get("subtrees", 0) >= 512, plans
    w = np.concatenate([s.read_rest(0)["weight"], s.read_rest(1)["weight"]])
    assert np.array_equal(w, ref.w0), "the system's weights are not its reference's"
    check_solves(s, ref, x, m3)


# ---------------------------------------------------------------- CPU: the host check of a record ----
@pytest.fixture(scope="module")
def br():
    os.makedirs(os.path.join(HERE, "_build"), exist_ok=True)
    out = os.path.join(HERE, "_build", "libbwdrecord.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "bwd_record_shim.cpp")])
    lib = C.CDLL(out)
    lib.br_check.argtypes = [C.POINTER(C.c_int), C.c_longlong, C.c_longlong, C.c_longlong, C.c_char_p, C.c_int]
    return lib


N_NODES, PANELS = 1000, 10000
NAMES = ("LEVELS", "NMEM", "MEM0", "NTASK", "TASK0", "XBUF", "VBUF", "END", "NSTAGE", "STAGE0", "HDR", "K", "R", "FIRST", "XOFF", "VOFF", "ROW0", "POFF", "MEM")


def small_record(br):
    """a root (8 columns at node 100, rows 300 and 301 above the subtree, x kept at offset 0) over one leaf (5 columns at node 50; rows:
    columns 0 and 3 of the root, and node 200 above the subtree) -> (record, the layout constants)"""
    c = {n: br.br_const(i) for i, n in enumerate(NAMES)}
    nl, nm = 2, 2
    mem0 = (c["HDR"] + 3 * (nl + 1) + 3) & ~3
    task0 = mem0 + c["MEM"] * nm
    tasks = [0 * 16 + 0, 0 * 16 + 1, 1 * 16 + 0, 1 * 16 + 1]
    stage0 = task0 + len(tasks)

    def w(node): return -1 - (2 * node + 1)       # a member's own column: from W

    def above(node): return -1 - 2 * node         # a row above the subtree: from global X
    stage = [w(100 + j) for j in range(8)] + [above(300), above(301)] + [w(50 + j) for j in range(5)] + [0, 9, above(200)]
    n_ints = (stage0 + len(stage) + 3) & ~3
    rec = np.zeros(n_ints, dtype=np.int32)
    xbuf = n_ints // 2
    vbuf = xbuf + 3 * 8
    rec[[c["LEVELS"], c["NMEM"], c["MEM0"], c["NTASK"], c["TASK0"], c["XBUF"], c["VBUF"], c["END"], c["NSTAGE"], c["STAGE0"]]] = \
        [nl, nm, mem0, len(tasks), task0, xbuf, vbuf, vbuf + 3 * 10, len(stage), stage0]
    rec[c["HDR"]:c["HDR"] + 3] = [0, 1, 2]
    rec[c["HDR"] + 3:c["HDR"] + 6] = [0, 2, 4]
    rec[c["HDR"] + 6:c["HDR"] + 9] = [0, 10, 18]
    for q, (k, r, first, xoff, row0, poff) in enumerate([(8, 2, 100, 0, 0, 0), (5, 3, 50, -1, 10, 80)]):
        M = mem0 + c["MEM"] * q
        rec[[M + c["K"], M + c["R"], M + c["FIRST"], M + c["XOFF"], M + c["VOFF"], M + c["ROW0"], M + c["POFF"], M + c["POFF"] + 1]] = [k, r, first, xoff, 0, row0, poff, 0]
    rec[task0:task0 + len(tasks)] = tasks
    rec[stage0:stage0 + len(stage)] = stage
    return rec, dict(c, mem0=mem0, task0=task0, stage0=stage0)


def verdict(br, rec):
    msg = C.create_string_buffer(256)
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    ok = br.br_check(rec.ctypes.data_as(C.POINTER(C.c_int)), rec.size, N_NODES, PANELS, msg, 256)
    return ok, msg.value.decode()


def test_record_check_refuses_corrupted_records(br):
    """the host check accepts the hand-written record, and refuses it with one out-of-range offset (a row beyond the x area; a staged
    vector beyond the workgroup's LDS) and with one column written twice (a task repeated in place of another; two members sharing an
    x slot); a row that names a member of its own level is refused too"""
    rec, c = small_record(br)
    ok, msg = verdict(br, rec)
    assert ok == 1, msg
    M1 = c["mem0"] + c["MEM"]

    def refused(edit, word):
        bad = rec.copy()
        edit(bad)
        ok, msg = verdict(br, bad)
        print(msg)
        assert ok == 0 and msg.startswith("backward subtree record: ") and word in msg, (ok, msg)

    def row_beyond_x(r): r[c["stage0"] + 10 + 6] = 3 * 8          # the leaf's second front row: one slot past the root's eight columns
    def stage_beyond_lds(r): r[M1 + c["VOFF"]] = 3 * 3            # the leaf's 8 rows from slot 3 of a 10-slot staging area
    def task_twice(r): r[c["task0"] + 3] = r[c["task0"] + 2]      # the leaf's columns 0..3 twice, 4 never
    def shared_x_slot(r): r[M1 + c["XOFF"]] = 3 * 3               # the leaf keeps its x in the root's slots 3..7
    def own_level_row(r): r[c["stage0"] + 8] = 0                  # the root reads x of its own column
    refused(row_beyond_x, "row outside the x area")
    refused(stage_beyond_lds, "staging offset")
    refused(task_twice, "column written twice")
    refused(shared_x_slot, "x slot written twice")
    refused(own_level_row, "not at a higher level")
