"""The child-pair node records (cuda-raytracer_amd/host/bvh_records.cpp: what SceneDev uploads and the
traversal kernels read) on hand-built trees, on the CPU: tests/native/bvh_records_test.cpp is a stand-alone
program over the same source the library links, built here with AddressSanitizer and UBSan.

Cases: a root leaf (no records); a three-node tree (record 0 + padding); seven and eleven nodes (siblings'
records an even/odd pair, pairs handed out depth-first with child1's subtree first); leaves of 63 / 64
triangles and begin >= 2^24 (inline ref / big-leaf table); a left-deep chain with its deepest internal node
at depth 31 (accepted) and 32 (refused); child indices -1 and node_count, a node that is its own descendant;
and for every record of every accepted tree unpack() against the children's bounds with memcmp (bounds
include -0.0, a denormal and inf).  The reference keeps one 32-B node per BVH node (scene.cuh); the records
are this port's layout, so its own definition (bvh_records.h) is what is checked."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HOST = os.path.join(REPO, "cuda-raytracer_amd", "host")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvh_records") / "bvh_records_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "include"), "-I", HOST,
                    os.path.join(HERE, "native", "bvh_records_test.cpp"), os.path.join(HOST, "bvh_records.cpp"),
                    "-o", out], check=True)
    return out


def test_bvh_records(prog):
    p = subprocess.run([prog], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok ") and "FAILED" not in p.stdout, p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
