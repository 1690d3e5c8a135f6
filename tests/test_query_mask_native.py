"""The host model of the low-complexity mask (ghostm_amd/csrc/query_mask_host.cpp,
query_mask.h) as a stand-alone program under AddressSanitizer and UBSan: random
sources through tile layouts against an independent evaluation, the runs of
more than 128 low windows with a single trigger at either end, the plan and the
refusals. It runs directly, with nothing preloaded. The device side runs the
same model in test_gpu_query_mask.py."""
import os
import subprocess


def test_query_mask_host_model_sanitized(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "native", "test_query_mask.cpp")
    model = os.path.join(os.path.dirname(here), "ghostm_amd", "csrc", "query_mask_host.cpp")
    exe = str(tmp_path / "test_query_mask")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    model, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
