"""The plan of both triangular sweeps (csrc/sweep_plan.hpp: plan_fused_subtrees, plan_levels, plan_shard_exchange), executed without a
GPU: tests/cpp/sweep_plan.cpp, a stand-alone program compiled with g++ together with csrc/factor.cpp and csrc/dense.cpp and run.  For
every case -- binary, four-way and eight-way trees, LDS caps that leave subtrees per-level in one or both sweeps, the fused launches
switched off, block items low in the tree with every kernel shape, padded item lists, forests, two subtree shards -- it plans a grid
Laplacian's factor, runs the plan on the CPU the way the kernels run it (fused records, level items, roots, stage tables) on panels and
right-hand sides from {-1, 0, 1}, and demands panel_solve_host's x bit for bit, every W, contribution and x entry written exactly once,
and every record and kernel shape within what the launches allow."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "admm-elastic-sca_amd", "csrc")


def test_sweep_plan_executed_against_panel_solve_host(tmp_path):
    exe = str(tmp_path / "sweep_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-psabi", "-fopenmp", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "sweep_plan.cpp"), os.path.join(CSRC, "factor.cpp"), os.path.join(CSRC, "dense.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "sweep_plan: ok" in r.stdout, r.stdout + r.stderr
