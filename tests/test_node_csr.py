"""build_node_csr (csrc/node_csr.hpp), the per-node lists of the gradient and reaction gathers, against brute-force per-node lists:
tests/cpp/node_csr.cpp, a stand-alone program that includes the header alone, compiled with g++ and run.  Its cases: 5 nodes and two
batches, a node that no element names, a node named twice by one element, an empty batch, n_nodes = 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_node_csr_against_brute_force(tmp_path):
    exe = str(tmp_path / "node_csr")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "admm-elastic-sca_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "node_csr.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "node_csr: ok" in r.stdout, r.stdout + r.stderr
