"""The subject pile-up's host plan (ghostm_amd/csrc/pileup_plan.h, host code):
compiled with g++ and checked on random spans and on the edge cases (a span
ending on a tile's last position, one starting on a tile's first, one over
three tiles, empty paths) — every (hit, tile) incidence exactly once, parts of
at most P hits in hit order, windows of whole tiles within the budget. The
same program also runs under -fsanitize=address,undefined. The device side
runs the plan in test_gpu_pileup.py."""
import os
import subprocess

import pytest

SRC = os.path.join(os.path.dirname(__file__), "native", "test_pileup_plan.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_pileup_plan(flags, tmp_path):
    exe = str(tmp_path / "test_pileup_plan")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
