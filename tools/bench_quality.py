"""Cost of the quality stage (k_qual_trim) next to the format kernel of the same
set: --reads synthetic DNA reads of --read-nt letters (200 000 x 150 by default)
with a quality profile of a high plateau, a decaying 3' tail and a few low 5'
letters, as a tiled DNA set of width 127 with -Q 20,10,30.

One session; the first set is left out (buffers grow, code objects load), then
--reps sets follow. Prints one JSON line: per repeat `seconds_query_format` and
`seconds_quality`, and what the stage did.

    python tools/bench_quality.py [--reads 200000] [--read-nt 150] [--reps 3] [--trim 20 --mask 10 --min-len 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main() -> None:
    import numpy as np

    from ghostm_amd.aligner import Session

    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--read-nt", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trim", type=int, default=20)
    ap.add_argument("--mask", type=int, default=10)
    ap.add_argument("--min-len", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    n, L = a.reads, a.read_nt
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, L))]
    q = rng.integers(30, 41, size=(n, L))
    tail = rng.integers(0, L // 3, size=n)            # the decaying 3' tail's length
    pos = np.arange(L)[None, :]
    in_tail = pos >= (L - tail)[:, None]
    q = np.where(in_tail, rng.integers(2, 22, size=(n, L)), q)
    q[:, :2] = np.where(rng.random((n, 2)) < 0.3, 2, q[:, :2])
    q = np.where(rng.random((n, L)) < 0.01, 5, q)     # random dips
    quals = (q + 33).astype(np.uint8)
    seqs = [bytes(r) for r in letters]
    qs = [bytes(r) for r in quals]
    names = [b"r%d" % k for k in range(n)]
    runs = []
    with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
        s.set_quality(a.trim, a.mask, a.min_len)
        for rep in range(a.reps + 1):
            s.set_queries(seqs, names, width=381, dna=True, tile_step=64, quals=qs)
            if rep:
                runs.append((s.stats()["seconds_query_format"], s.quality_stats()["seconds_quality"]))
        st = s.quality_stats()
    print(json.dumps({"case": "quality", "reads": n, "read_nt": L, "params": [a.trim, a.mask, a.min_len],
                      "seconds_query_format": [r[0] for r in runs], "seconds_quality": [r[1] for r in runs],
                      "stats": {k: v for k, v in st.items() if k != "seconds_quality"}}))


if __name__ == "__main__":
    main()
