"""Time the read-level rows post-pass (k_read_rows; -y 14, Session.hits_band_rows)
beside k_path_rows on the same hits' tile paths in the same session.

The workload is tools/bench_band.py's: protein reads of 300-600 letters set
tiled (width 127, step 64) against a preset's database. One -y 7 session; the
first run is left out, then --repeat runs, after each of which hits_rows() (the
tile paths' rows, k_path_rows) and hits_band_rows() (the band paths' rows,
k_read_rows<false>) are taken and the two passes' device seconds, launches and
columns read from the session's counters. With --frame-reads N the same for
tools/bench_frame.py's DNA reads and hits_frame_rows() (k_read_rows<true>).
Prints one JSON line with the build's source hash.

    python tools/bench_read_rows.py --preset cfg3 --reads 200000 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench_band  # noqa: E402
import bench_frame  # noqa: E402
from ghostm_amd import native, srchash, workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402


def measure(s, repeat: int, frame: bool) -> list:
    runs = []
    for k in range(repeat + 1):
        s.run()
        tile, _ = s.hits_rows()
        rec, _ = s.hits_frame_rows() if frame else s.hits_band_rows()
        st, rr = s.stats(), s.read_rows_stats()
        bs = s.frame_stats() if frame else st  # stats() carries the band pass's counters
        if k:
            runs.append({
                "hits": int(len(rec)), "seconds_path_rows": st["seconds_path_rows"],
                "path_rows_launches": st["path_rows_launches"], "path_rows_columns": st["path_rows_columns"],
                "seconds_read_rows": rr["seconds_read_rows"], "read_rows_launches": rr["read_rows_launches"],
                "read_rows_columns": rr["read_rows_columns"],
                "seconds_path_pass": bs["seconds_frame" if frame else "seconds_band"],
                "shift_columns": int(rec["shifts"].sum()),
                "rescore_equals_score": bool((rec["rescore"] == (s.hits_frame() if frame else s.hits_band())[0]["score"]).all()),
                "tile_columns": int(tile["columns"].sum()),
            })
    return runs


def summary(runs: list) -> dict:
    best = min(runs, key=lambda r: r["seconds_read_rows"])
    rd, tl = best["seconds_read_rows"], best["seconds_path_rows"]
    return {
        "seconds_read_rows": rd, "seconds_path_rows": tl, "ratio_to_path_rows": rd / tl if tl else None,
        "read_columns_per_s": best["read_rows_columns"] / rd if rd else None,
        "path_columns_per_s": best["path_rows_columns"] / tl if tl else None,
        "row_bytes_per_s": 3 * best["read_rows_columns"] / rd if rd else None,
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--frame-reads", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_read_rows")
    args = ap.parse_args()
    w = workloads.WORKLOADS[args.preset]
    root = os.path.join(args.workdir, args.preset, "db")
    os.makedirs(root, exist_ok=True)
    fasta = os.path.join(root, "subjects.fa")
    if w["db"][0] == "synth":
        workloads._run(workloads.GHOSTM, "synth", "-d", fasta, "-N", str(w["db"][1]), "-s", str(w["db"][2]))
    else:
        fasta = w["db"][1]
    db = os.path.join(root, "db")
    workloads._run(workloads.GHOSTM, "db", "-i", fasta, "-o", db)
    subjects = bench_band.subjects_of(fasta, 50_000)
    info = (native.load().GhostmBuildInfo() or b"").decode()
    out = {"preset": args.preset, "width": 127, "step": 64, "source_hash": srchash.tree_hash(),
           "library_hash": srchash.info_hash(info)}
    reads = bench_band.make_reads(subjects, args.reads)
    with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", "7"]) as s:
        s.set_queries(reads, [f"r{i}" for i in range(len(reads))], width=127, tile_step=64)
        out["band"] = {"reads": len(reads), "letters": sum(len(x) for x in reads), "runs": measure(s, args.repeat, False)}
        out["band"]["best"] = summary(out["band"]["runs"])
    if args.frame_reads:
        reads = bench_frame.make_reads(subjects, args.frame_reads)
        with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", "7"]) as s:
            s.set_queries(reads, [f"r{i}" for i in range(len(reads))], width=3 * 127, dna=True, tile_step=64)
            out["frame"] = {"reads": len(reads), "nt": sum(len(x) for x in reads), "runs": measure(s, args.repeat, True)}
            out["frame"]["best"] = summary(out["frame"]["runs"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
