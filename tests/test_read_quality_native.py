"""The host model of the quality stage (ghostm_amd/csrc/read_quality_host.cpp,
read_quality.h) and the FASTQ reader (fastq_reader.cpp) as a stand-alone program
under AddressSanitizer and UBSan: random reads at odd offsets against an
independent O(n^2) evaluation of the rule, the refusals, and the reader on
well-formed, CRLF, truncated and mismatched files. It runs directly, with
nothing preloaded. The device side runs the same model in
test_gpu_read_quality.py."""
import os
import subprocess


def test_read_quality_host_model_and_reader_sanitized(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "ghostm_amd", "csrc")
    src = os.path.join(here, "native", "test_read_quality.cpp")
    exe = str(tmp_path / "test_read_quality")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    os.path.join(csrc, "read_quality_host.cpp"), os.path.join(csrc, "fastq_reader.cpp"), "-o", exe],
                   check=True)
    files = tmp_path / "files"
    files.mkdir()
    r = subprocess.run([exe, str(files)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all ok" in r.stdout
