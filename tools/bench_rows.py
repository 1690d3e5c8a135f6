"""Time the aligned-rows post-pass (-y 8, k_path_rows) against the path
post-pass it sits behind (-y 7).

For one preset (ghostm_amd/workloads.py): a resident session per style, the
first run left out, then --repeat runs each; per run the session's stats of the
post-passes and the step time. From the -y 8 runs: the row bytes per second of
device time, as a fraction of the HBM figure, the ratio to the path kernels'
time of the same run, and the host bytes held for the rows. Prints one JSON line.

    python tools/bench_rows.py --preset cfg4 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ghostm_amd import HIT_ROWS_DTYPE, workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E
KEYS = ("seconds_total", "seconds_traceback_ext", "seconds_traceback_path", "traceback_path_launches",
        "seconds_path_rows", "path_rows_launches", "path_rows_columns", "path_rows_bytes", "hits")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg4")
    ap.add_argument("--queries", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_rows")
    args = ap.parse_args()
    w = workloads.WORKLOADS[args.preset]
    n = args.queries or w["queries"]
    root = os.path.join(args.workdir, args.preset)
    db = workloads.make_db(args.preset, os.path.join(root, "db"))
    q = workloads.make_queries(args.preset, os.path.join(root, "q"), 0, n)
    out = {"preset": args.preset, "queries": n}
    for y in ("7", "8"):
        runs = []
        with Session(["-i", q, "-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", y]) as s:
            for k in range(args.repeat + 1):
                t = time.perf_counter()
                s.run()
                wall = time.perf_counter() - t
                st = s.stats()
                if k:
                    runs.append(dict({key: st[key] for key in KEYS}, wall=wall))
            if y == "8":
                rec, rows = s.hits_rows()
                out["rows_records"] = int(len(rec))
                out["rows_host_bytes"] = int(len(rows)) + int(len(rec)) * HIT_ROWS_DTYPE.itemsize
                out["columns_per_hit"] = float(rec["columns"].mean()) if len(rec) else 0.0
                out["gapped_hits"] = int((rec["gap_residues"] > 0).sum())
                out["output_bytes"] = len(s.output())
        out["y" + y] = runs
    best = min(out["y8"], key=lambda r: r["seconds_path_rows"])
    sec = best["seconds_path_rows"]
    out["rows_kernel"] = {
        "seconds": sec, "bytes": best["path_rows_bytes"],
        "bytes_per_s": best["path_rows_bytes"] / sec if sec else None,
        "fraction_of_hbm_peak": best["path_rows_bytes"] / sec / HBM_PEAK if sec else None,
        "ratio_to_path_kernels": sec / best["seconds_traceback_path"] if best["seconds_traceback_path"] else None,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
