"""The host model of the mate-pair join (ghostm_amd/csrc/pair_join_host.cpp,
pair_join.h) as a stand-alone program under AddressSanitizer and UBSan: random
calls against an evaluation that sorts the list of every concordant pair of
hits, the contract's largest values, and every refusal with the outputs
untouched. It runs directly, with nothing preloaded. The device side runs the
same model in test_gpu_pair_join.py."""
import os
import subprocess


def test_pair_join_host_model_sanitized(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "native", "test_pair_join.cpp")
    model = os.path.join(os.path.dirname(here), "ghostm_amd", "csrc", "pair_join_host.cpp")
    exe = str(tmp_path / "test_pair_join")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    model, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
