"""Device time of the tiled query formatter (k_qry_frames_tiled) beside the
untiled one (k_qry_frames) on the same letters: 200 K synthetic reads of 300-600
nt set six times each on one database session, `seconds_query_format` of every
set. Prints one JSON line.

    python tools/bench_tiles.py"""
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from ghostm_amd.aligner import Session  # noqa: E402

N = 200_000
r = random.Random(1)
# a pool of random letters, reads cut from it (making 90 M random letters in Python takes too long)
pool = "".join(r.choice("ACGT") for _ in range(1 << 20))
reads = []
for i in range(N):
    n = r.randint(300, 600)
    a = r.randrange(0, len(pool) - n)
    reads.append(pool[a:a + n])
names = [f"r{i}" for i in range(N)]
letters = sum(len(x) for x in reads)

with tempfile.TemporaryDirectory() as tmp:
    db = os.path.join(tmp, "db")
    subprocess.run([os.path.join(REPO, "ghostm_amd", "bin", "ghostm"), "db", "-i",
                    os.path.join(REPO, "tests", "golden", "testset_queries.fasta"), "-o", db], check=True,
                   capture_output=True)
    res = {"reads": N, "nt": letters}
    with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"]) as s:
        for label, kw in (("untiled_w381", dict(width=381)), ("tiled_w381_step64", dict(width=381, tile_step=64)),
                          ("tiled_w381_step127", dict(width=381, tile_step=127)),
                          ("tiled_w381_step16", dict(width=381, tile_step=16))):
            times, rows = [], 0
            for k in range(6):
                s.set_queries(reads, names, dna=True, **kw)
                st = s.stats()
                times.append(st["seconds_query_format"] * 1e3)
                rows = len(s.query_lengths())
            res[label] = {"rows": rows, "bytes_out": rows * 127, "launches": st["query_format_launches"],
                          "ms_first": round(times[0], 4), "ms_min": round(min(times[1:]), 4),
                          "ms_median": round(statistics.median(times[1:]), 4), "ms_max": round(max(times[1:]), 4)}
    print(json.dumps(res))
