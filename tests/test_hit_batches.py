"""The per-hit detail passes' host arithmetic (ghostm_amd/csrc/hit_batches.h,
host code): compiled with g++ and checked on random hit arrays — the column
counts of the extended and the path traceback, their launch order (the stable
sort by column count), the batch cuts of the path traceback and the rows
(in order, at least one hit, within the hit cap and the byte budget, maximal),
the batch counts the GPU tests pin (GHOSTM_PATH_BATCH_HITS=7 and
GHOSTM_ROWS_BATCH_HITS=7 on 60 hits) and every refusal's text. The device
side runs them in test_gpu_traceback_ext.py, test_gpu_traceback_path.py and
test_gpu_path_rows.py."""
import os
import subprocess


def test_hit_batches(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "native", "test_hit_batches.cpp")
    exe = str(tmp_path / "test_hit_batches")
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
