"""Time a query set replaced on a live database session against a fresh process.

For one preset (ghostm_amd/workloads.py): the database session's creation,
set_queries_fasta (wall, and the formatting kernels' device time), set_queries
from records already in memory (no FASTA parse), the run after each set, and on
the same visit a cold `ghostm aln` process on pre-formatted files, `ghostm qry`
+ `ghostm aln`, and `ghostm search` with one and with two pairs. The outputs
are compared byte for byte. Prints one JSON line.

    python tools/bench_search.py --preset cfg4 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ghostm_amd import workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def read_fasta(path):
    names, seqs = [], []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                names.append(line[1:].lstrip(b"> "))
                seqs.append([])
            elif names and line:
                seqs[-1].append(line)
    return [b"".join(s) for s in seqs], names


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg4")
    ap.add_argument("--queries", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_search")
    args = ap.parse_args()
    w = workloads.WORKLOADS[args.preset]
    n = args.queries or w["queries"]
    root = os.path.join(args.workdir, args.preset)
    os.makedirs(root, exist_ok=True)
    db = workloads.make_db(args.preset, os.path.join(root, "db"))
    fa = os.path.join(root, "q.fa")
    subprocess.run([workloads.GHOSTM, "synth", "-q", fa, "-n", str(n), "-f", "0", *w["synth"]], check=True,
                   capture_output=True)
    qopt = list(w["qry"])
    width = int(qopt[qopt.index("-l") + 1]) if "-l" in qopt else 75
    dna = "-t" in qopt and qopt[qopt.index("-t") + 1] == "d"
    q = os.path.join(root, "q")
    aln = list(w["aln"])
    out = {"preset": args.preset, "queries": n, "fasta_bytes": os.path.getsize(fa)}

    # fresh processes, same visit: qry, then a cold aln on its files; and search
    t_qry, _ = timed(lambda: subprocess.run([workloads.GHOSTM, "qry", "-i", fa, "-o", q] + qopt, check=True,
                                            capture_output=True))
    cold, t_search = [], []
    for k in range(args.repeat):
        t, _ = timed(lambda: subprocess.run([workloads.GHOSTM, "aln", "-i", q, "-d", db, "-o",
                                             os.path.join(root, "aln.out")] + aln, check=True, capture_output=True))
        cold.append(t)
        t, _ = timed(lambda: subprocess.run(
            [workloads.GHOSTM, "search", "-w", str(width), "-q", "d" if dna else "p", "-d", db] + aln
            + [fa, os.path.join(root, "search.out")], check=True, capture_output=True))
        t_search.append(t)
    # two pairs in one process: what a second read set costs
    t_two, _ = timed(lambda: subprocess.run(
        [workloads.GHOSTM, "search", "-w", str(width), "-q", "d" if dna else "p", "-d", db] + aln
        + [fa, os.path.join(root, "search.out"), fa, os.path.join(root, "search2.out")], check=True,
        capture_output=True))
    out["search_two_pairs_process_s"] = t_two
    want = open(os.path.join(root, "aln.out"), "rb").read()
    out["qry_process_s"] = t_qry
    out["aln_cold_process_s"] = cold
    out["qry_plus_aln_s"] = t_qry + min(cold)
    out["search_process_s"] = t_search
    out["search_output_equals_aln"] = open(os.path.join(root, "search.out"), "rb").read() == want

    t_create, s = timed(lambda: Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + aln))
    out["create_db_session_s"] = t_create
    sets = []
    with s:
        for k in range(args.repeat):
            t_set, cut = timed(lambda: s.set_queries_fasta(fa, width=width, dna=dna))
            st = s.stats()
            t_run, _ = timed(s.run)
            t_run2, _ = timed(s.run)
            sets.append({"set_queries_fasta_s": t_set, "seconds_query_read": st["seconds_query_read"],
                         "seconds_query_load": st["seconds_query_load"],
                         "seconds_query_format": st["seconds_query_format"],
                         "query_format_launches": st["query_format_launches"], "run_after_set_s": t_run,
                         "second_run_s": t_run2, "output_equals_aln": s.output() == want, "cut_records": cut})
        records = s.query_lengths().size
        rec_bytes = sum(s.query_records(c).size for c in range(st["query_format_launches"]))
        t_parse, (seqs, names) = timed(lambda: read_fasta(fa))
        mem = []
        for k in range(args.repeat):
            t_set, _ = timed(lambda: s.set_queries(seqs, names, width=width, dna=dna))
            st2 = s.stats()
            mem.append({"set_queries_s": t_set, "seconds_query_load": st2["seconds_query_load"],
                        "seconds_query_format": st2["seconds_query_format"]})
        t_run, _ = timed(s.run)
        out["set_queries_output_equals_aln"] = s.output() == want
        out["query_sets"] = s.stats()["query_sets"]
    out["sets_from_fasta"] = sets
    out["sets_from_memory"] = mem
    out["python_fasta_parse_s"] = t_parse
    # the kernels' traffic: the letters a record can contribute, 8 + 4 bytes of
    # offset and length per input record, the coded records and 4 bytes of length each
    per = 6 if dna else 1
    cap = None if dna else width
    letters = sum(len(x) if cap is None else min(len(x), min(cap, 127)) for x in seqs)
    nbytes = letters * (per if dna else 1) + 12 * len(seqs) + rec_bytes + 4 * records
    fmt = min(x["seconds_query_format"] for x in sets)
    out["format_kernel"] = {"bytes": nbytes, "seconds": fmt, "bytes_per_s": nbytes / fmt if fmt else None,
                            "fraction_of_hbm_peak": nbytes / fmt / HBM_PEAK if fmt else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
