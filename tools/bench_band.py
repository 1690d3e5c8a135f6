"""Time the read-level band post-pass (-y 12; k_band_fill<false>,
k_band_walk<false>, k_ops_compact) beside the per-tile path post-pass it sits behind (-y 7).

Protein reads of 300-600 letters: a random flank, a 140-400 letter stretch of
a subject of a preset's database (ghostm_amd/workloads.py) copied at an 8 %
substitution rate, a third of them with one planted indel of 1-6 letters, a
random flank. They are set tiled (width 127, step 64) on one resident database
session per style; the first run is left out, then --repeat runs each. Per run:
the session's stats of the two post-passes and the step time. From the -y 12
runs: band cells per second of device time, direction bytes, the band pass
beside seconds_traceback_path of the same run, and how many read-level paths
are longer than a record. Prints one JSON line.

    python tools/bench_band.py --preset cfg3 --reads 200000 --workdir /tmp/data --repeat 3
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

from ghostm_amd import workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

AA = "ARNDCQEGHILKMFPSTWYV"
KEYS = ("seconds_total", "seconds_traceback_ext", "seconds_traceback_path", "traceback_path_launches",
        "traceback_path_cells", "seconds_band", "band_launches", "band_hits", "band_cells", "band_dir_bytes", "hits")


def subjects_of(fasta: str, limit: int) -> list:
    out, cur = [], []
    with open(fasta) as f:
        for line in f:
            if line.startswith(">"):
                if cur:
                    out.append("".join(cur))
                    cur = []
                    if len(out) >= limit:
                        break
            else:
                cur.append(line.strip())
    if cur and len(out) < limit:
        out.append("".join(cur))
    return [s for s in out if len(s) >= 150]


def make_reads(subjects: list, n: int, seed: int = 1) -> list:
    r = random.Random(seed)
    pool = "".join(r.choice(AA) for _ in range(1 << 20))  # the flanks are cut from one pool of random letters
    reads = []
    for i in range(n):
        sub = subjects[r.randrange(len(subjects))]
        span = min(r.randint(140, 400), len(sub))
        a = r.randrange(0, len(sub) - span + 1)
        core = list(sub[a:a + span])
        for _ in range(span * 8 // 100):
            core[r.randrange(span)] = r.choice(AA)
        core = "".join(core)
        if i % 3 == 0:
            p, k = r.randint(15, span - 15), r.randint(1, 6)
            core = core[:p] + pool[p:p + k] + core[p:] if r.random() < 0.5 else core[:p] + core[p + k:]
        total = max(r.randint(300, 600), len(core))
        left = r.randint(0, total - len(core))
        b = r.randrange(0, len(pool) - total)
        reads.append(pool[b:b + left] + core + pool[b + left:b + total - len(core)])
    return reads


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--band", type=int, default=31)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_band")
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
    reads = make_reads(subjects_of(fasta, 50_000), args.reads)
    names = [f"r{i}" for i in range(len(reads))]
    out = {"preset": args.preset, "reads": len(reads), "letters": sum(len(x) for x in reads), "band": args.band,
           "width": 127, "step": 64}
    for y in ("7", "12"):
        runs = []
        with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", y]) as s:
            s.set_band(args.band)
            s.set_queries(reads, names, width=127, tile_step=64)
            out["tile_records"] = int(len(s.query_lengths()))
            for k in range(args.repeat + 1):
                t = time.perf_counter()
                s.run()
                wall = time.perf_counter() - t
                st = s.stats()
                if k:
                    runs.append(dict({key: st[key] for key in KEYS}, wall=wall))
            if y == "12":
                rec, ops = s.hits_band()
                path, pops = s.hits_path()
                # columns per hit from the words (a prefix sum keeps this off the per-word Python path)
                csum = np.concatenate([[0], np.cumsum(ops >> 4, dtype=np.int64)])
                off = rec["ops_offset"].astype(np.int64)
                cols = csum[off + rec["n_runs"]] - csum[off]
                out["band_records"] = int(len(rec))
                out["columns_per_hit"] = float(cols.mean()) if len(rec) else 0.0
                out["paths_over_127_columns"] = int((cols > 127).sum())
                out["score_above_tile_path"] = int((rec["score"] > path["score"]).sum())
                below = np.flatnonzero(rec["score"] < path["score"])
                out["score_below_tile_path"] = int(len(below))
                # ... of which the tile path stays within the band of its first cell (the band pass promises
                # at least the tile path's score for these): its drift, 'D' columns minus 'I' columns so far
                inside = 0
                for h in below.tolist():
                    drift, ok = 0, True
                    for w in pops[int(path["ops_offset"][h]):int(path["ops_offset"][h]) + int(path["n_runs"][h])]:
                        n, op = int(w) >> 4, int(w) & 3
                        drift += n if op == 3 else -n if op == 2 else 0
                        ok = ok and abs(drift) <= args.band
                    inside += ok
                out["score_below_tile_path_inside_band"] = inside
                out["output_bytes"] = len(s.output())
        out["y" + y] = runs
    best = min(out["y12"], key=lambda r: r["seconds_band"])
    sec = best["seconds_band"]
    out["band_kernels"] = {
        "seconds": sec, "cells": best["band_cells"], "dir_bytes": best["band_dir_bytes"],
        "cells_per_s": best["band_cells"] / sec if sec else None,
        "ratio_to_path_kernels": sec / best["seconds_traceback_path"] if best["seconds_traceback_path"] else None,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
