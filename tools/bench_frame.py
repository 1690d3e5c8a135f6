"""Time the frameshift-aware read-level post-pass (-y 13; k_band_fill<true>,
k_band_walk<true>, k_ops_compact) beside the band pass (-y 12) and the per-tile
path pass on the same hits of the same session.

DNA reads of 900-1800 nt: a random flank, a 140-400 residue stretch of a
subject of a preset's database (ghostm_amd/workloads.py) back-translated with
one fixed codon per residue at an 8 % substitution rate, two thirds of them with
one or two planted single-nucleotide insertions or deletions, a random flank;
every other read reverse-complemented. The codons are chosen so that the
off-frames of a back-translated stretch hold a stop codon only after a
methionine: the tiled setters mask a frame from a stop codon to its next ATG,
and a frame masked before the indel cannot be followed after it. The reads are
set tiled (width 381 nt = 127 letters, step 64) on one resident database session
per style; the first run is left out, then --repeat runs each. After every -y 13
run the band results of the same hits are taken too. Prints one JSON line.

    python tools/bench_frame.py --preset cfg3 --reads 50000 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ghostm_amd import workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

AA = "ARNDCQEGHILKMFPSTWYV"
CODON = dict(A="GCC", R="CGC", N="AAC", D="GAC", C="TGC", Q="CAG", E="GAG", G="GGC", H="CAC", I="ATC", L="CTC",
             K="AAG", M="ATG", F="TTC", P="CCC", S="AGC", T="ACC", W="TGG", Y="TAC", V="GTC")
KEYS = ("seconds_total", "seconds_traceback_path", "traceback_path_cells", "seconds_band", "band_hits", "band_cells",
        "band_dir_bytes", "hits")


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


def back_translate(prot: str) -> str:
    return "".join(CODON.get(c, "GCC") for c in prot)


def make_reads(subjects: list, n: int, seed: int = 1) -> list:
    r = random.Random(seed)
    pool = back_translate("".join(r.choice(AA) for _ in range(1 << 18)))  # the flanks are cut from one pool
    flip = str.maketrans("ACGT", "TGCA")
    reads = []
    for i in range(n):
        sub = subjects[r.randrange(len(subjects))]
        span = min(r.randint(140, 400), len(sub))
        a = r.randrange(0, len(sub) - span + 1)
        core = list(sub[a:a + span])
        for _ in range(span * 8 // 100):
            core[r.randrange(span)] = r.choice(AA)
        core = back_translate("".join(core))
        for _ in range(i % 3):  # 0, 1 or 2 single-nucleotide indels
            p = r.randint(45, len(core) - 45)
            core = core[:p] + r.choice("ACGT") + core[p:] if r.random() < 0.5 else core[:p] + core[p + 1:]
        total = max(r.randint(900, 1800), len(core))
        left = r.randint(0, total - len(core))
        b = r.randrange(0, len(pool) - total)
        dna = pool[b:b + left] + core + pool[b + left:b + total - len(core)]
        reads.append(dna[::-1].translate(flip) if i % 2 else dna)
    return reads


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--band", type=int, default=31)
    ap.add_argument("--shift", type=int, default=15, help="the frameshift cost (non-negative)")
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_frame")
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
    out = {"preset": args.preset, "reads": len(reads), "nucleotides": sum(len(x) for x in reads), "band": args.band,
           "shift": -args.shift, "width": 127, "step": 64}
    for y in ("12", "13"):
        runs = []
        with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", y]) as s:
            s.set_band(args.band)
            s.set_frame_shift(-args.shift)
            s.set_queries(reads, names, width=381, dna=True, tile_step=64)
            out["tile_records"] = int(len(s.query_lengths()))
            for k in range(args.repeat + 1):
                t = time.perf_counter()
                s.run()
                wall = time.perf_counter() - t
                if y == "13":
                    s.hits_band()  # the band pass on the same hits of the same session
                st = s.stats()
                if k:
                    runs.append(dict({key: st[key] for key in KEYS}, wall=wall, **s.frame_stats()))
            if y == "13":
                rec, ops = s.hits_frame()
                band = s.hits_band()[0]
                info = s.frame_info()
                out["frame_records"] = int(len(rec))
                out["frame_score_above_band"] = int((rec["score"] > band["score"]).sum())
                out["frame_score_below_band"] = int((rec["score"] < band["score"]).sum())
                out["hits_with_shifts"] = int((info["shifts"] > 0).sum())
                out["shifts"] = int(info["shifts"].sum())
                out["reverse_strand_hits"] = int(info["strand"].sum())
                out["output_bytes"] = len(s.output())
        out["y" + y] = runs
    best = min(out["y13"], key=lambda r: r["seconds_frame"])
    sec = best["seconds_frame"]
    out["frame_kernels"] = {
        "seconds": sec, "cells": best["frame_cells"], "dir_bytes": best["frame_dir_bytes"],
        "cells_per_s": best["frame_cells"] / sec if sec else None,
        "band_seconds": best["seconds_band"],
        "band_cells_per_s": best["band_cells"] / best["seconds_band"] if best["seconds_band"] else None,
        "ratio_to_band_kernels": sec / best["seconds_band"] if best["seconds_band"] else None,
        "ratio_to_path_kernels": sec / best["seconds_traceback_path"] if best["seconds_traceback_path"] else None,
        "share_frame_above_band": out["frame_score_above_band"] / max(out["frame_records"], 1),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
