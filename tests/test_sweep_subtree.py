"""The bottom subtrees of the elimination tree swept by one launch per sweep, one workgroup per subtree (sweep_plan.hpp plan_fused_subtrees,
solve_fwd_subtree_kernel): the same x, BIT FOR BIT, as the per-level launches (ADMM_HIP_SWEEP_FUSE=0) -- after one solve and after
whole frames -- on the headline bar, the mixed scene and a two-rank subtree-sharded run on one GPU.  Every case also asserts from the
sweep plan (ADMM_HIP_VERBOSE) that subtrees were fused at all, so that a comparison of the per-level path with itself cannot pass.
"""
import re
import threading

import numpy as np
import pytest

PLAN = re.compile(r"admm_hip: plan fused cut (\d+) subtrees (\d+) left (\d+) lds (\d+) cap (\d+)")


def _plans(err):
    return [dict(zip(("cut", "subtrees", "left", "lds", "cap"), map(int, m.groups()))) for m in PLAN.finditer(err)]


def _pair(monkeypatch, capfd, make):
    """(per-level system, fused system, the fused one's plan lines), both initialized"""
    out = []
    for fuse in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE", fuse)
        monkeypatch.setenv("ADMM_HIP_VERBOSE", fuse)
        capfd.readouterr()
        s = make()
        s.initialize()
        out.append(s)
        err = capfd.readouterr().err
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    return out[0], out[1], _plans(err)


def _same_solves_and_frames(ref, fused, frames, iters):
    rng = np.random.default_rng(7)
    n = ref.info()["n_nodes"]
    for _ in range(2):
        b = rng.standard_normal(3 * n)
        assert np.array_equal(ref.solve_only(b), fused.solve_only(b))
    for f in range(frames):
        ref.step(iters); fused.step(iters)
        assert np.array_equal(ref.m_x, fused.m_x), ("frame", f)
        assert np.array_equal(ref.m_v, fused.m_v), ("frame", f)


@pytest.mark.gpu
def test_headline_bar_bitwise(pkg, monkeypatch, capfd):
    """the 1M-tet bar: three fused levels (cut 2)"""
    ref, fused, plans = _pair(monkeypatch, capfd, lambda: pkg.make_bar_system(32, 32, 163))
    assert plans and plans[0]["cut"] >= 2 and plans[0]["subtrees"] >= 512, plans
    _same_solves_and_frames(ref, fused, frames=2, iters=10)


@pytest.mark.gpu
def test_mixed_scene_bitwise(pkg, monkeypatch, capfd):
    """NH + StVK tets and a cloth with hinges in one system"""
    ref, fused, plans = _pair(monkeypatch, capfd, lambda: pkg.make_mixed_system(26, 26, 123, 158, 158)[0])
    assert plans and plans[0]["subtrees"] > 0, plans
    _same_solves_and_frames(ref, fused, frames=2, iters=10)


@pytest.mark.gpu
def test_two_subtree_shards_on_one_gpu_bitwise(pkg, monkeypatch, capfd):
    """subtree sharding, two ranks on one GPU (threads + an in-process all-reduce): every rank fuses its own bottom subtrees; the
    ranks' x equal each other and the per-level run's, bit for bit"""
    import torch
    dims = (32, 32, 163)
    runs, plans = {}, []
    for fuse in ("0", "1"):
        monkeypatch.setenv("ADMM_HIP_SWEEP_FUSE", fuse)
        monkeypatch.setenv("ADMM_HIP_VERBOSE", fuse)
        monkeypatch.setenv("ADMM_HIP_SHARD", "subtree")
        capfd.readouterr()
        shards = [pkg.make_bar_system(*dims, rank=r, world=2, shard_mode=1) for r in range(2)]
        bar = threading.Barrier(2)
        bufs = {}

        class _Ptr:
            def __init__(self, ptr, count):
                self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        def make_hook(r):
            def hook(ptr, count, stream):
                torch.cuda.synchronize()
                bufs[r] = torch.as_tensor(_Ptr(ptr, count), device="cuda:0")
                bar.wait()
                if r == 0:
                    tot = bufs[0] + bufs[1]
                    bufs[0].copy_(tot); bufs[1].copy_(tot)
                    torch.cuda.synchronize()
                bar.wait()
                return 0
            return hook
        for r, s in enumerate(shards):
            s.set_allreduce(make_hook(r))
        pkg.initialize_together(shards)
        plans += _plans(capfd.readouterr().err) if fuse == "1" else []
        errs = []

        def run(s):
            try:
                s.step(10); s.sync()
            except Exception as e:    # surface failures of a worker thread
                errs.append(e)
        xs = []
        for frame in range(2):
            th = [threading.Thread(target=run, args=(s,)) for s in shards]
            [t.start() for t in th]; [t.join() for t in th]
            assert not errs, errs
            assert np.array_equal(shards[0].m_x, shards[1].m_x), (fuse, frame)
            xs.append(shards[0].m_x.copy())
        runs[fuse] = xs
        del shards
    monkeypatch.delenv("ADMM_HIP_VERBOSE")
    assert len(plans) == 2 and all(p["subtrees"] > 0 for p in plans), plans
    for a, b in zip(runs["0"], runs["1"]):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_subtrees_over_the_lds_cap_stay_per_level(pkg, monkeypatch, capfd):
    """a long bar cut at level 3 (four fused levels): a few of its subtrees need more LDS than leaves two workgroups per CU and keep
    their per-level launches next to the fused one -- and the result is still bit for bit the same"""
    ref, fused, plans = _pair(monkeypatch, capfd, lambda: pkg.make_bar_system(24, 24, 400))
    assert plans and plans[0]["subtrees"] > 0 and plans[0]["left"] > 0, plans
    _same_solves_and_frames(ref, fused, frames=1, iters=10)
