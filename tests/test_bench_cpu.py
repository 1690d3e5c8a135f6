"""bench.py's all-cores CPU figure: the reference CPU path split
over processes by contiguous query ranges must give the one-process output
byte for byte (queries are independent; names are unique per synthetic query)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GHOSTM = os.path.join(REPO, "ghostm_amd", "bin", "ghostm")
CPU_EXES = [os.path.join(REPO, "oracle", "_ref", "ghostm_ref"), os.path.join(REPO, "oracle", "_build", "ghostm_oracle")]


@pytest.mark.skipif(not os.path.exists(GHOSTM) or not any(os.path.exists(p) for p in CPU_EXES),
                    reason="CLI or CPU oracle not built (run __graft_entry__.build())")
@pytest.mark.parametrize("preset,procs", [("cfg2", 1), ("cfg2", 3), ("cfg3", 4)])
def test_cpu_split_matches_one_process(tmp_path, preset, procs):
    import bench
    from ghostm_amd import workloads

    w = str(tmp_path)
    nq = 90
    db = workloads.make_db(preset, os.path.join(w, "db"))
    q = workloads.make_queries(preset, os.path.join(w, "one"), 0, nq)
    exe = next(p for p in CPU_EXES if os.path.exists(p))
    aln = workloads.WORKLOADS[preset]["aln"]
    subprocess.run([exe, "aln", "-i", q, "-d", db, "-o", f"{w}/one.out"] + aln, check=True, capture_output=True)
    one = open(f"{w}/one.out", "rb").read()
    assert one
    joined, dt, nparts, per = bench.reference_split(os.path.join(w, "split"), preset, db, nq, aln, procs)
    assert nparts == procs and dt > 0
    assert joined == one


def test_dump_outputs_arrays(tmp_path, monkeypatch):
    """--dump-outputs: float arrays only, every record and byte while they fit, a
    fixed sample (the same from call to call) once they do not."""
    import hashlib

    import numpy as np

    import bench
    from ghostm_amd.aligner import HIT_DTYPE

    # the largest dump (both samples full) stays under 64 MB with room for the small arrays
    assert bench.DUMP_HIT_ROWS * (len(HIT_DTYPE.names) + 1) * 8 + bench.DUMP_TEXT_BYTES * (4 + 8) < 63_000_000
    hits = np.zeros(37, dtype=HIT_DTYPE)
    hits["query_id"] = np.arange(37)
    hits["score"] = 0xFFFFFFFF - np.arange(37)  # u32 values are exact in float64
    hits["seq_id"] = np.linspace(0, 1, 37, dtype=np.float32)
    text = bytes(range(256)) * 3 + b"tail\n"

    def load(d):
        return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}

    bench.dump_outputs(str(tmp_path / "a"), text, hits)
    a = load(str(tmp_path / "a"))
    assert set(a) == {"hits", "hits_rows", "hits_count", "output_text", "output_text_offsets", "output_bytes",
                      "output_sha256"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["hits"].shape == (37, len(HIT_DTYPE.names)) and a["hits_count"][0] == 37
    for j, name in enumerate(HIT_DTYPE.names):
        assert (a["hits"][:, j] == hits[name]).all()
    assert a["output_text"].astype(np.uint8).tobytes() == text and a["output_bytes"][0] == len(text)
    assert a["output_sha256"].astype(np.uint8).tobytes() == hashlib.sha256(text).digest()

    monkeypatch.setattr(bench, "DUMP_HIT_ROWS", 10)
    monkeypatch.setattr(bench, "DUMP_TEXT_BYTES", 100)
    bench.dump_outputs(str(tmp_path / "b"), text, hits)
    bench.dump_outputs(str(tmp_path / "c"), text, hits)
    b, c = load(str(tmp_path / "b")), load(str(tmp_path / "c"))
    assert all((b[k] == c[k]).all() for k in b)
    rows, offs = b["hits_rows"].astype(int), b["output_text_offsets"].astype(int)
    assert len(rows) == 10 and (np.diff(rows) > 0).all() and b["hits_count"][0] == 37
    assert (b["hits"][:, 0] == hits["query_id"][rows]).all()
    assert len(offs) == 100 and (np.diff(offs) > 0).all()
    assert b["output_text"].astype(np.uint8).tobytes() == bytes(text[i] for i in offs)
    assert (b["output_sha256"] == a["output_sha256"]).all()


def test_full_pin_only_for_the_full_workload():
    import bench
    from ghostm_amd import workloads

    pins = bench._json(bench.FULL_GOLDEN) or {}
    for name, w in workloads.WORKLOADS.items():
        if name in pins:
            assert bench.full_pin(name, w["queries"], list(w["aln"])) is not None
        assert bench.full_pin(name, w["queries"] - 1, list(w["aln"])) is None
        assert bench.full_pin(name, w["queries"], list(w["aln"]) + ["-b", "3"]) is None
