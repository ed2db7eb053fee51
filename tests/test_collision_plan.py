"""collision_form_of and plan_mesh_tables (csrc/collision_plan.hpp), the host's pure planning of the collision meshes:
tests/cpp/collision_plan.cpp, a stand-alone program that includes the header alone, compiled with g++ and run.  The form: a hand-written
table of lists and mesh facts -- the empty list, analytic shapes with and without an unnamed mesh, each of the seven triggers alone and
with the one below it, a motion without a coefficient, a body surface's coefficient, a box without a frame, form 7 without the latch, a
trigger in entry n, the same mesh twice.  The tables: against brute force per node and mesh -- 7 nodes under a non-identity permutation,
four meshes of which two share an owner range, a self-colliding sheet and body, two meshes with side memory, and the cases without an
owner, without self-collision, without meshes and with n_nodes = 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_collision_plan_against_table_and_brute_force(tmp_path):
    exe = str(tmp_path / "collision_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "admm-elastic-sca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "collision_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "collision_plan: ok" in r.stdout, r.stdout + r.stderr
