"""Time the read-level cull (k_read_cull; -y 20 / -y 21, Session.read_cull) beside
the band and frame passes whose records it reads.

tools/bench_band.py's protein reads (300-600 letters) and tools/bench_frame.py's
DNA reads are set tiled (width 127 / 381, step 64) on one resident database
session of a preset (ghostm_amd/workloads.py), with tile groups off and on. The
first run is left out, then --repeat runs each; after every run read_cull() is
taken (band paths for the protein reads, frame paths for the DNA reads). Per
run: seconds_cull beside seconds_band / seconds_frame, the launches, the hits by
status, and the reads by the kernel's size class (at most 64, 256, 1024 hits,
more). Prints one JSON line.

    python tools/bench_cull.py --preset cfg3 --reads 200000 --dna-reads 10000 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench_band  # noqa: E402
import bench_frame  # noqa: E402
from ghostm_amd import workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

CLASSES = (64, 256, 1024)


def read_sizes(s: Session) -> np.ndarray:
    """hits per read: runs of hits of one source record (a hit's query_id is the
    last record of its group, a tile of the read the resolved record is a tile of)"""
    rec = s.query_tiles()["record"][s.hits()["query_id"]]
    if not len(rec):
        return np.zeros(0, dtype=np.int64)
    cut = np.flatnonzero(np.diff(rec.astype(np.int64)) != 0) + 1
    return np.diff(np.concatenate([[0], cut, [len(rec)]]))


def measure(db, aln, reads, dna, groups, repeat, sizes):
    names = [f"r{i}" for i in range(len(reads))]
    runs = []
    with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + aln + ["-y", "7"]) as s:
        s.set_tile_groups(groups)
        s.set_queries(reads, names, width=381 if dna else 127, dna=dna, tile_step=64)
        for k in range(repeat + 1):
            t = time.perf_counter()
            s.run()
            search = time.perf_counter() - t
            t = time.perf_counter()
            if dna:
                s.hits_frame()
            else:
                s.hits_band()
            paths = time.perf_counter() - t
            t = time.perf_counter()
            out = s.read_cull(dna)
            wall_cull = time.perf_counter() - t
            if not k:
                continue
            st, frame = s.read_cull_stats(), s.frame_stats()
            runs.append(dict(st, seconds_band=s.stats()["seconds_band"], seconds_frame=frame["seconds_frame"],
                             wall_search=search, wall_paths=paths, wall_cull=wall_cull,
                             empty=int((out["status"] == 3).sum())))
        if sizes:
            n = read_sizes(s)
            hist = [int((n <= CLASSES[0]).sum())] + [int(((n > a) & (n <= b)).sum()) for a, b in zip(CLASSES, CLASSES[1:])]
            return runs, {"reads_with_hits": int(len(n)), "at_most_64_256_1024": hist, "more": int((n > CLASSES[-1]).sum()),
                          "largest": int(n.max()) if len(n) else 0}
    return runs, None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--dna-reads", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_cull")
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
    sets = {"protein": (bench_band.make_reads(subjects, args.reads), False),
            "dna": (bench_frame.make_reads(subjects, args.dna_reads), True)}
    out = {"preset": args.preset, "width": 127, "step": 64, "top_k": 1, "cover_pct": 50}
    for name, (reads, dna) in sets.items():
        if not reads:
            continue
        for groups in (False, True):
            runs, hist = measure(db, list(w["aln"]), reads, dna, groups, args.repeat, True)
            out[f"{name}_groups_{'on' if groups else 'off'}"] = {"reads": len(reads), "runs": runs, "read_sizes": hist}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
