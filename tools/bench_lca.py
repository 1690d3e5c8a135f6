"""Time the per-read taxonomic assignment (k_read_lca_wave / k_read_lca; -y 22 /
-y 23, Session.read_lca) beside the cull and the band and frame passes whose
records it reads.

tools/bench_cull.py's workload (tools/bench_band.py's protein reads and
tools/bench_frame.py's DNA reads, set tiled with tile groups on, on one resident
database session of a preset) with a synthetic taxonomy over the database's
subjects: a seeded random tree of depth about 30 with the subjects on its
leaves. The first run is left out, then --repeat runs each; after every run
read_cull() and then read_lca() are taken (band paths for the protein reads,
frame paths for the DNA reads). Per run: seconds_lca beside seconds_cull and
seconds_band / seconds_frame, the wall time of the read_lca() call and the share
of it spent on the host, the launches, votes and assigned reads, and the reads
by the kernel's size class (at most 64, 1024 candidates, more). Prints one JSON
line.

    python tools/bench_lca.py --preset cfg3 --reads 200000 --dna-reads 10000 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench_band  # noqa: E402
import bench_frame  # noqa: E402
from ghostm_amd import taxonomy_depths, workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402


def synthetic_taxonomy(nsubjects: int, seed: int = 20261208, depth: int = 20):
    """(taxid, parent, subject_node): inner nodes in a random tree whose mean
    step to the parent is 1 / depth of the nodes (the deepest node comes out
    about 30 levels down for depth 20), then one leaf per subject under a random
    inner node"""
    rnd = random.Random(seed)
    inner = max(64, nsubjects // 8)
    window = max(2, 2 * inner // depth)
    parent = [0] + [rnd.randrange(max(0, k - window), k) for k in range(1, inner)]
    parent += [rnd.randrange(inner) for _ in range(nsubjects)]
    n = len(parent)
    return (np.arange(1, n + 1, dtype=np.uint32), np.array(parent, dtype=np.uint32),
            np.arange(inner, n, dtype=np.uint32))


def measure(db, aln, reads, dna, tax, repeat):
    names = [f"r{i}" for i in range(len(reads))]
    runs = []
    with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + aln + ["-y", "7"]) as s:
        s.set_tile_groups(True)
        s.set_taxonomy(*tax)
        s.set_queries(reads, names, width=381 if dna else 127, dna=dna, tile_step=64)
        for k in range(repeat + 1):
            s.run()
            s.hits_frame() if dna else s.hits_band()
            s.read_cull(dna)
            t = time.perf_counter()
            out = s.read_lca(dna)
            wall = time.perf_counter() - t
            if not k:
                continue
            st, frame = s.read_lca_stats(), s.frame_stats()
            runs.append(dict(st, seconds_cull=s.read_cull_stats()["seconds_cull"], seconds_band=s.stats()["seconds_band"],
                             seconds_frame=frame["seconds_frame"], wall_lca=wall,
                             host_share=1.0 - st["seconds_lca"] / wall if wall else 0.0))
        c = out["candidates"].astype(np.int64)
        hist = {"reads": int(len(c)), "at_most_64_1024": [int((c <= 64).sum()), int(((c > 64) & (c <= 1024)).sum())],
                "more": int((c > 1024).sum()), "largest": int(c.max()) if len(c) else 0,
                "mean_depth": float(out["depth"][out["votes"] > 0].mean()) if (out["votes"] > 0).any() else 0.0}
    return runs, hist


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--dna-reads", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_lca")
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
    with open(fasta, "rb") as f:
        nsubjects = sum(line.startswith(b">") for line in f)
    tax = synthetic_taxonomy(nsubjects)
    subjects = bench_band.subjects_of(fasta, 50_000)
    sets = {"protein": (bench_band.make_reads(subjects, args.reads), False),
            "dna": (bench_frame.make_reads(subjects, args.dna_reads), True)}
    out = {"preset": args.preset, "width": 127, "step": 64, "top_pct": 10, "support_pct": 100, "subjects": nsubjects,
           "nodes": int(len(tax[0])), "tree_depth": int(taxonomy_depths(tax[1]).max())}
    for name, (reads, dna) in sets.items():
        if not reads:
            continue
        runs, hist = measure(db, list(w["aln"]), reads, dna, tax, args.repeat)
        out[name] = {"reads": len(reads), "runs": runs, "read_candidates": hist}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
