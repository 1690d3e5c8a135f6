"""The per-read passes' batch plan (ghostm_amd/csrc/read_classes.h, host code):
compiled with g++ and checked on reads of sizes 0, 1, 64, 65, 256, 257, 1024,
1025 and 3000, in that order and under seeded shuffles, with the cull's class
bounds and the LCA's, with and without the size arrays — every read with a size
lies in exactly one list, in read order, in its size's class (a size equal to a
bound in the lower one), a read of size 0 in none, and the meta words are the
layout the kernels index: the read_begin slice, the lists, the padding to an
even word, the u64 table offsets. The device side runs the plan in
test_gpu_read_cull.py and test_gpu_read_lca.py."""
import os
import subprocess


def test_read_classes(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "native", "test_read_classes.cpp")
    exe = str(tmp_path / "test_read_classes")
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
