"""Time the read-level subject pile-up (k_read_pileup; -y 16, Session.read_pileup)
beside the tile pile-up (k_pileup; -y 10, Session.pileup) on the same run's
hits in the same session.

The workload is tools/bench_band.py's: protein reads of 300-600 letters set
tiled (width 127, step 64) against a preset's database. One -y 7 session; the
first run is left out, then --repeat runs, after each of which pileup() (the
tile paths, k_pileup) and read_pileup(False) (the band paths,
k_read_pileup<false>) are taken and the two passes' device seconds, launches,
parts and columns read from the session's counters. With --frame-reads N the
same for tools/bench_frame.py's DNA reads and read_pileup(True)
(k_read_pileup<true>). No threshold: the read-level pass charges more columns
per hit and walks a hit once per tile it meets. Prints one JSON line with the
build's source hash and, with --out, writes it there too.

    python tools/bench_read_pileup.py --preset cfg3 --reads 200000 --workdir /tmp/data --repeat 3
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
        tile = s.pileup()
        read = s.read_pileup(frame)
        st, rp = s.stats(), s.read_pileup_stats()
        if k:
            runs.append({
                "hits": int(read[0]["hits"].sum()), "positions": int(len(read[1])),
                "seconds_pileup": st["seconds_pileup"], "pileup_launches": st["pileup_launches"],
                "pileup_windows": st["pileup_windows"], "pileup_parts": st["pileup_parts"],
                "pileup_columns": st["pileup_columns"],
                **rp,
                "tile_covered": int(tile[0]["covered"].sum()), "read_covered": int(read[0]["covered"].sum()),
                "depth_sum_equals_columns": bool(int(read[0]["depth_sum"].sum()) == rp["read_pileup_columns"]),
            })
    return runs


def summary(runs: list) -> dict:
    best = min(runs, key=lambda r: r["seconds_read_pileup"])
    rd, tl = best["seconds_read_pileup"], best["seconds_pileup"]
    return {
        "seconds_read_pileup": rd, "seconds_pileup": tl, "ratio_to_pileup": rd / tl if tl else None,
        "read_columns": best["read_pileup_columns"], "tile_columns": best["pileup_columns"],
        "column_ratio": best["read_pileup_columns"] / best["pileup_columns"] if best["pileup_columns"] else None,
        "read_columns_per_s": best["read_pileup_columns"] / rd if rd else None,
        "tile_columns_per_s": best["pileup_columns"] / tl if tl else None,
        "parts_ratio": best["read_pileup_parts"] / best["pileup_parts"] if best["pileup_parts"] else None,
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg3")
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--frame-reads", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_read_pileup")
    ap.add_argument("--out", default="")
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
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
