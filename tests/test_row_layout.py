"""row_blocks, blocks_before, block_row and partial_blocks_bound (csrc/row_layout.hpp), the rule that places the 64-item blocks of the
per-entry and per-body partial sums: tests/cpp/row_layout.cpp, a stand-alone program that includes the header alone, compiled with g++
and run.  Totals from {0, 1, 63, 64, 65, 128} over 0 .. ADMM_MAX_SHAPES + 1 rows against a brute-force count: every block below the sum
maps to exactly one row, the first at or beyond it to none."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_layout_against_brute_force(tmp_path):
    exe = str(tmp_path / "row_layout")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "admm-elastic-sca_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "row_layout.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "row_layout: ok" in r.stdout, r.stdout + r.stderr
