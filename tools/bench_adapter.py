"""Cost of the adapter stage (k_adapter_find + k_pair_overlap) next to the quality
stage and the format kernel of the same set: --pairs synthetic pairs of DNA
mates of --read-nt letters (200 000 x 2 x 150 by default). About a third are
read through: a fragment of 40..read_nt-1 letters, then the TruSeq adapter of
its mate, then random letters, with 1 % wrong letters. The set goes in as a
tiled DNA set of width 127 with -A both adapters, -O 5,10,20 and -Q 20,10,30.

One session; per setting the first set is left out (buffers grow, code objects
load), then --reps sets follow. Three settings, so that the time divides
between the kernels: both rules, the adapter rule alone, the pair rule alone.
Prints one JSON line: per repeat `seconds_query_format`, `seconds_quality` and
`seconds_adapter`, and what the stage did.

    python tools/bench_adapter.py [--pairs 200000] [--read-nt 150] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ADAPTER1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def make_pairs(n: int, L: int, seed: int = 13):
    """(letters, quality bytes, names) of 2 n records, mates interleaved, and the read-through pairs' count"""
    import numpy as np

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    frag = rng.integers(0, 4, size=(n, L))                      # the fragment's first L letters, as codes
    through = rng.random(n) < 1 / 3
    flen = np.where(through, rng.integers(40, L, size=n), L)    # its length; L: no read-through seen
    pos = np.arange(L)[None, :]
    mates = []
    for k, adapter in enumerate((ADAPTER1, ADAPTER2)):
        if k == 0:
            own = frag
        else:  # mate 2 reads the fragment's other strand from its far end (for a whole fragment: any other letters)
            idx = np.clip(flen[:, None] - 1 - pos, 0, L - 1)
            own = np.where(through[:, None], 3 - np.take_along_axis(frag, idx, axis=1), rng.integers(0, 4, size=(n, L)))
        ad_codes = np.concatenate([np.array([b"ACGT".index(c) for c in adapter]), rng.integers(0, 4, size=L)])
        tail = ad_codes[np.clip(pos - flen[:, None], 0, ad_codes.size - 1)]  # the adapter, then random letters
        codes = np.where(pos < flen[:, None], own, tail)
        wrong = rng.random((n, L)) < 0.01
        codes = np.where(wrong, (codes + rng.integers(1, 4, size=(n, L))) % 4, codes)
        mates.append(acgt[codes])
    q = rng.integers(30, 41, size=(2 * n, L))
    tailq = rng.integers(0, L // 3, size=2 * n)
    q = np.where(pos >= (L - tailq)[:, None], rng.integers(2, 22, size=(2 * n, L)), q)
    quals = (q + 33).astype(np.uint8)
    seqs = [bytes(mates[r & 1][r >> 1]) for r in range(2 * n)]
    qs = [bytes(r) for r in quals]
    names = [b"p%d/%d" % (r >> 1, 1 + (r & 1)) for r in range(2 * n)]
    return seqs, qs, names, int(through.sum())


def main() -> None:
    from ghostm_amd.aligner import Session

    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--read-nt", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n, L = a.pairs, a.read_nt
    seqs, qs, names, through = make_pairs(n, L)
    settings = {"both": (ADAPTER1, ADAPTER2, 5, 10, 20), "adapter_rule": (ADAPTER1, ADAPTER2, 5, 10, 0),
                "pair_rule": (b"", b"", 5, 10, 20)}
    res = {"case": "adapter", "pairs": n, "read_nt": L, "read_through_pairs": through}
    with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
        s.set_quality(20, 10, 30)
        for name, params in settings.items():
            s.set_adapters(*params)
            runs = []
            for rep in range(a.reps + 1):
                s.set_queries(seqs, names, width=381, dna=True, tile_step=64, quals=qs)
                if rep:
                    runs.append((s.stats()["seconds_query_format"], s.quality_stats()["seconds_quality"],
                                 s.adapter_stats()["seconds_adapter"]))
            st = s.adapter_stats()
            res[name] = {"seconds_query_format": [r[0] for r in runs], "seconds_quality": [r[1] for r in runs],
                         "seconds_adapter": [r[2] for r in runs],
                         "stats": {k: v for k, v in st.items() if k != "seconds_adapter"}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
