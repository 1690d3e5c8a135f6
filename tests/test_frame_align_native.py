"""The frame pass's host arithmetic (ghostm_amd/csrc/frame_align.h, host code):
compiled with g++ and checked on random hits — the nucleotide rows a band runs
against a scan of every row, the three frames' letter addressing against the
tile plan, the scratch formula, the word bound against random walks, and the
refusals it adds. The device side runs them in test_gpu_frame_align.py."""
import os
import subprocess


def test_frame_align_arithmetic(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "native", "test_frame_align.cpp")
    exe = str(tmp_path / "test_frame_align")
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
