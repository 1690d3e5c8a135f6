"""Time a database replaced on a live session against the path through files.

For one preset (ghostm_amd/workloads.py; its database FASTA, a sample of its
queries): --repeat set_db_fasta calls on one session (wall, and the split into
FASTA reading, host loading, the coding kernel and the index build), a run
after each set, and on the same visit what the files cost for the same FASTA:
a `ghostm db -D 0` process, then Session.for_db on its files. For the coding
kernel the bytes moved per second (the packed letters read, the codes written)
against the HBM peak and against what a device-to-device copy reaches; for the
resident index build its device time against GhostmBuildIndexGpu's device_ms
on the same residues in the same process (they share the launch sequence). The
outputs are compared byte for byte. Prints one JSON line (and writes it to
--out).

    python tools/bench_setdb.py --preset cfg4 --workdir /tmp/data --repeat 3
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from ghostm_amd import native, workloads  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, MI355X HBM3E
HBM_COPY = 6.3e12   # bytes/s read + written, what a device-to-device copy reaches


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="cfg4")
    ap.add_argument("--queries", type=int, default=20000, help="queries of the runs after each set")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--index-reps", type=int, default=5)
    ap.add_argument("--workdir", default="/tmp/ghostm_bench_setdb")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = workloads.WORKLOADS[args.preset]
    if w["db"][0] != "synth":
        raise SystemExit("bench_setdb: a preset with a generated database (cfg3, cfg4, cfg5)")
    _, residues, seed = w["db"]
    root = os.path.join(args.workdir, args.preset)
    os.makedirs(root, exist_ok=True)
    fa = os.path.join(root, "db.fa")
    subprocess.run([workloads.GHOSTM, "synth", "-d", fa, "-N", str(residues), "-s", str(seed)], check=True,
                   capture_output=True)
    q = workloads.make_queries(args.preset, os.path.join(root, "queries"), 0, args.queries)
    aln = list(w["aln"])
    out = {"preset": args.preset, "db_residues": residues, "fasta_bytes": os.path.getsize(fa),
           "queries": args.queries}

    # the path through files: a formatter process (index on the GPU), then a session on its files
    db = os.path.join(root, "db")
    files = []
    for _ in range(args.repeat):
        t_db, _ = timed(lambda: subprocess.run([workloads.GHOSTM, "db", "-i", fa, "-o", db, "-D", "0"], check=True,
                                               capture_output=True))
        t_create, s = timed(lambda: Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"] + aln))
        s.close()
        files.append({"db_process_s": t_db, "create_db_session_s": t_create, "sum_s": t_db + t_create})
    out["through_files"] = files
    with Session(["-i", q, "-d", db, "-o", os.devnull, "-D", "0"] + aln) as s:
        s.run()
        want = s.output()
        t_run_files, _ = timed(s.run)
    out["run_on_files_s"] = t_run_files

    sets = []
    with Session.for_queries(["-i", q, "-o", os.devnull, "-D", "0"] + aln) as s:
        for _ in range(args.repeat):
            t_set, _ = timed(lambda: s.set_db_fasta(fa))
            st = s.stats()
            t_run, _ = timed(s.run)
            t_run2, _ = timed(s.run)
            sets.append({"set_db_fasta_s": t_set, "seconds_db_read": st["seconds_db_read"],
                         "seconds_db_load": st["seconds_db_load"], "seconds_db_code": st["seconds_db_code"],
                         "seconds_db_index": st["seconds_db_format"] - st["seconds_db_code"],
                         "db_format_launches": st["db_format_launches"], "run_after_set_s": t_run,
                         "second_run_s": t_run2, "output_equals_files": s.output() == want})
        chunks = s.db_chunks()
        out["db_chunks"] = chunks
        out["db_sets"] = s.stats()["db_sets"]
        out["pool_cached_bytes_after_sets"] = native.device_pool_info()[0]
        # the stand-alone build on the same residues, in this process
        seq = s.db_records(0)
        c = chunks[0]
        kc = np.zeros(c["kcl"], dtype=np.uint32)
        pos = np.zeros(len(seq), dtype=np.uint32)
        npos = ctypes.c_uint32(0)
        u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))  # noqa: E731
        alone = []
        for _ in range(args.index_reps):
            ms = ctypes.c_float(0)
            if native.load().GhostmBuildIndexGpu(seq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(seq),
                                                 c["seed"], c["kcl"], u32(kc), u32(pos), ctypes.byref(npos), 0,
                                                 ctypes.byref(ms)):
                raise RuntimeError(native.last_error())
            alone.append(ms.value * 1e-3)
        _, kc_res, pos_res = s.db_index(0)
        out["index_equals_stand_alone"] = bool(npos.value == c["npos"] and kc_res.tobytes() == kc.tobytes()
                                               and pos_res.tobytes() == pos[:npos.value].tobytes())
    out["sets"] = sets
    nbytes = 2 * sum(x["len"] for x in chunks)  # every byte read once and written once
    code = min(x["seconds_db_code"] for x in sets)
    out["coding_kernel"] = {"bytes": nbytes, "seconds": code, "seconds_all": [x["seconds_db_code"] for x in sets],
                            "bytes_per_s": nbytes / code if code else None,
                            "fraction_of_hbm_peak": nbytes / code / HBM_PEAK if code else None,
                            "fraction_of_copy_rate": nbytes / code / HBM_COPY if code else None}
    resident = [x["seconds_db_index"] for x in sets]
    out["index_build"] = {"resident_s": resident, "stand_alone_s": alone,
                          "resident_min_s": min(resident), "stand_alone_min_s": min(alone),
                          "stand_alone_max_s": max(alone),
                          "resident_inside_stand_alone_spread": bool(min(alone) <= min(resident) <= max(alone)),
                          "chunks_in_resident_figure": len(chunks)}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
