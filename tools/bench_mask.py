"""Cost of the low-complexity mask pass (k_mask_windows + k_mask_apply) next to
the format kernel of the same set: tools/bench_qry.py's protein set (1M synthetic
queries, cfg4's) and its DNA read count (200 000 reads, here --read-nt long so
that a frame spans tiles), both as tiled sets of width 127 with masking on.

One session per case; the first set of the session is left out (buffers grow,
code objects load), then --reps sets follow. Prints one JSON line per case: per
repeat `seconds_query_format` and `seconds_mask` of the set, the bytes both
passes move at least (format: letters read + records written + 12 B per source
record; mask: the sources' letters read once through the tiles + the two flag
words per 64 windows written and read + the masked bytes stored + 4 B per record
+ 20 B per source) against HBM peak, and what was masked.

    python tools/bench_mask.py [--queries 1000000] [--reads 200000] [--read-nt 600] [--reps 3]
                               [--window 12 --trigger 220 --extend 250]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK_HBM_GBS = 8000.0


def fasta_lengths(fa: str):
    import numpy as np

    lens = []
    with open(fa, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                lens.append(0)
            elif lens:
                lens[-1] += len(line.rstrip(b"\r\n"))
    return np.array(lens, dtype=np.int64)


def case(name: str, fa: str, width: int, dna: bool, step: int, reps: int, params) -> dict:
    from ghostm_amd.aligner import Session

    lens = fasta_lengths(fa)
    w = params[0]
    runs = []
    with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
        s.set_mask(*params)
        for rep in range(reps + 1):
            s.set_queries_fasta(fa, width=width, dna=dna, tile_step=step)
            st, ms = s.stats(), s.mask_stats()
            if rep == 0:
                continue  # the session's first set
            nq = len(s.query_lengths())
            W = width // 3 if dna else width
            fmt_bytes = int(lens.sum()) + nq * W + 12 * len(lens)
            letters = ms["mask_windows"] + (w - 1) * ms["mask_sources"]
            words = (ms["mask_windows"] + 63 * ms["mask_sources"]) // 64  # at most: every source rounds up
            stored = int(s.query_masked().sum(dtype="int64"))
            mask_bytes = letters + 2 * 16 * words + stored + 4 * nq + 20 * ms["mask_sources"]
            runs.append({
                "seconds_query_format": st["seconds_query_format"], "seconds_mask": ms["seconds_mask"],
                "format_bytes": fmt_bytes, "mask_bytes": mask_bytes,
                "format_gbs": fmt_bytes / st["seconds_query_format"] / 1e9,
                "mask_gbs": mask_bytes / ms["seconds_mask"] / 1e9 if ms["seconds_mask"] else None,
                "mask_over_format": ms["seconds_mask"] / st["seconds_query_format"],
                "chunks": ms["mask_launches"], "query_records": nq, **{k: ms[k] for k in (
                    "mask_sources", "mask_windows", "masked_sources", "masked_letters")},
                "masked_record_letters": stored, "masked_share_of_letters": ms["masked_letters"] / max(letters, 1),
            })
    best = min(runs, key=lambda r: r["seconds_mask"])
    return {"case": name, "records_in": len(lens), "width": width, "tile_step": step, "window": params[0],
            "trigger": params[1], "extend": params[2], "peak_hbm_gbs": PEAK_HBM_GBS,
            "best_mask_hbm_frac": best["mask_gbs"] / PEAK_HBM_GBS if best["mask_gbs"] else None,
            "best_format_hbm_frac": max(r["format_gbs"] for r in runs) / PEAK_HBM_GBS, "runs": runs}


def main() -> None:
    from ghostm_amd.native import BIN_PATH

    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--read-nt", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--trigger", type=int, default=220)
    ap.add_argument("--extend", type=int, default=250)
    args = ap.parse_args()
    params = (args.window, args.trigger, args.extend)
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([BIN_PATH, "synth", "-q", f"{tmp}/p.fa", "-n", str(args.queries), "-s", "4",
                        "-N", "10000000"], check=True, capture_output=True)
        print(json.dumps(case("protein_tiled", f"{tmp}/p.fa", 127, False, 64, args.reps, params)), flush=True)
        os.remove(f"{tmp}/p.fa")
        subprocess.run([BIN_PATH, "synth", "-q", f"{tmp}/d.fa", "-d", f"{tmp}/db.fa", "-n", str(args.reads),
                        "-N", "100000", "-s", "5", "-t", "dna", "-l", str(args.read_nt)], check=True, capture_output=True)
        print(json.dumps(case("dna_tiled", f"{tmp}/d.fa", 381, True, 64, args.reps, params)), flush=True)


if __name__ == "__main__":
    main()
