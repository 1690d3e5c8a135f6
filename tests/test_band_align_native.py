"""The band pass's host arithmetic (ghostm_amd/csrc/band_align.h, host code):
compiled with g++ and checked on random hits — the rows a band runs against a
scan of every row, the letter addressing through the tile records against the
tile plan, the scratch formulas, and every refusal's reason. The device side
runs them in test_gpu_band_align.py."""
import os
import subprocess


def test_band_align_arithmetic(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "native", "test_band_align.cpp")
    exe = str(tmp_path / "test_band_align")
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
