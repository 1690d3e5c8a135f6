"""The host model of the adapter stage (ghostm_amd/csrc/read_adapter_host.cpp,
read_adapter.h) as a stand-alone program under AddressSanitizer and UBSan:
random reads and pairs at odd offsets against an independent evaluation of the
rule on the letters themselves, mates at the 1024-letter limit, and the
refusals. It runs directly, with nothing preloaded. The device side runs the
same model in test_gpu_read_adapter.py."""
import os
import subprocess


def test_read_adapter_host_model_sanitized(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "ghostm_amd", "csrc")
    src = os.path.join(here, "native", "test_read_adapter.cpp")
    exe = str(tmp_path / "test_read_adapter")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    os.path.join(csrc, "read_adapter_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
