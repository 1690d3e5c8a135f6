"""Time the subject pile-up post-pass (-y 10, k_pileup + k_pileup_finish)
against the path post-pass it sits behind (-y 7) and against k_path_rows, which
walks the same columns of the same hits and so serves as the yardstick.

For one preset (ghostm_amd/workloads.py): a resident session per style, the
first run left out, then --repeat runs each; per run the session's stats of the
post-passes and the step time. From the -y 10 session also the rows' device
time on the same hits (hits_rows()), the subjects' summary, and, with --sweep,
the pile-up's device time for every GHOSTM_PILEUP_TILE x GHOSTM_PILEUP_PART_HITS
pair given (one more run each, the best of --repeat). Prints one JSON line.

    python tools/bench_pileup.py --preset cfg4 --workdir /tmp/data --repeat 3 --sweep 128,256:256,512
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ghostm_amd import workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

KEYS = ("seconds_total", "seconds_traceback_ext", "seconds_traceback_path", "seconds_path_rows", "path_rows_columns",
        "seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns", "hits")


def timed_run(s) -> dict:
    t = time.perf_counter()
    s.run()
    wall = time.perf_counter() - t
    st = s.stats()
    return dict({key: st[key] for key in KEYS}, wall=wall)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg4")
    ap.add_argument("--queries", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_pileup")
    ap.add_argument("--sweep", default="", help="tiles:parts, comma-separated values, e.g. 128,256:256,512")
    args = ap.parse_args()
    w = workloads.WORKLOADS[args.preset]
    n = args.queries or w["queries"]
    root = os.path.join(args.workdir, args.preset)
    db = workloads.make_db(args.preset, os.path.join(root, "db"))
    q = workloads.make_queries(args.preset, os.path.join(root, "q"), 0, n)
    out = {"preset": args.preset, "queries": n}
    for knob in ("GHOSTM_PILEUP_TILE", "GHOSTM_PILEUP_PART_HITS"):
        os.environ.pop(knob, None)
    for y in ("7", "10"):
        with Session(["-i", q, "-d", db, "-o", os.devnull, "-D", "0"] + list(w["aln"]) + ["-y", y]) as s:
            out["y" + y] = [timed_run(s) for k in range(args.repeat + 1)][1:]
            if y == "10":
                subj, depth, ident, cons = s.pileup()
                hit = subj[subj["hits"] > 0]
                out["subjects"] = int(len(subj))
                out["subjects_with_hits"] = int(len(hit))
                out["positions"] = int(len(depth))
                out["positions_covered"] = int(subj["covered"].sum())
                out["max_depth"] = int(subj["max_depth"].max()) if len(subj) else 0
                out["depth_sum"] = int(subj["depth_sum"].sum())
                out["identities_sum"] = int(subj["identities_sum"].sum())
                out["output_bytes"] = len(s.output())
                s.hits_rows()  # k_path_rows on the same hits
                st = s.stats()
                out["rows_same_hits"] = {"seconds": st["seconds_path_rows"], "columns": st["path_rows_columns"]}
                sweep = []
                if args.sweep:
                    tiles, parts = (x.split(",") for x in args.sweep.split(":"))
                    for t in tiles:
                        for p in parts:
                            os.environ["GHOSTM_PILEUP_TILE"], os.environ["GHOSTM_PILEUP_PART_HITS"] = t, p
                            runs = [timed_run(s) for k in range(args.repeat)]
                            best = min(runs, key=lambda r: r["seconds_pileup"])
                            sweep.append({"tile": int(t), "part_hits": int(p), "seconds_pileup": best["seconds_pileup"],
                                          "all_seconds": [r["seconds_pileup"] for r in runs],
                                          "parts": best["pileup_parts"], "launches": best["pileup_launches"]})
                    for knob in ("GHOSTM_PILEUP_TILE", "GHOSTM_PILEUP_PART_HITS"):
                        os.environ.pop(knob, None)
                out["sweep"] = sweep
    best = min(out["y10"], key=lambda r: r["seconds_pileup"])
    sec, rows = best["seconds_pileup"], out["rows_same_hits"]["seconds"]
    out["pileup_kernels"] = {
        "seconds": sec, "columns": best["pileup_columns"], "parts": best["pileup_parts"],
        "windows": best["pileup_windows"], "launches": best["pileup_launches"],
        "columns_per_s": best["pileup_columns"] / sec if sec else None,
        "ratio_to_path_rows": sec / rows if rows else None,
        "ratio_to_path_kernels": sec / best["seconds_traceback_path"] if best["seconds_traceback_path"] else None,
    }
    out["step_wall_s"] = {"y7": min(r["wall"] for r in out["y7"]), "y10": min(r["wall"] for r in out["y10"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
