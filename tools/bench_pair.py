"""Time the mate-pair join (k_pair_join; PairJoinGpu) beside the cull and the
assignment on the same records, at the stage level: no search runs.

Two synthetic record sets, seeded:
  short   --pairs pairs of short reads: one to four hits a mate on a handful of
          subjects, about two thirds of the pairs with a concordant hit
  large   --large-pairs pairs of 600 to 1024 hits (the LDS class)
Per set, after one call that is left out, --repeat calls each of
  ReadCullGpu  the same hits, every mate a read          (seconds_cull)
  PairJoinGpu  the hits as they are                      (seconds_pair)
  ReadLcaGpu   the joined candidates, every pair a read  (seconds_lca)
over a star taxonomy with one leaf per subject. Device seconds are the stage
counters'; the wall time of the join call is printed beside them. Prints one
JSON line per set.

    python tools/bench_pair.py --pairs 1000000 --large-pairs 4000 --repeat 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from ghostm_amd import (CULL_HIT_DTYPE, PAIR_HIT_DTYPE, pair_join, read_cull, read_lca, set_taxonomy_gpu,  # noqa: E402
                        stage_pair_join_stats, stage_read_cull_stats, stage_read_lca_stats)

SUBJECTS = 4096


def make_set(npairs: int, lo: int, hi: int, seed: int):
    """(pair_begin, offset, hits): every mate lo..hi hits; a pair's hits lie on
    four subjects of its own, mate 2 about 300 residues downstream on the other strand"""
    rng = np.random.default_rng(seed)
    per = rng.integers(lo, hi + 1, size=2 * npairs)
    begin = np.zeros(2 * npairs + 1, dtype=np.uint32)
    begin[1:] = np.cumsum(per)
    n = int(begin[-1])
    mate = np.repeat(np.arange(2 * npairs) & 1, per).astype(np.uint32)
    pair = np.repeat(np.arange(2 * npairs) >> 1, per)
    h = np.zeros(n, dtype=PAIR_HIT_DTYPE)
    h["subject"] = (pair * 7 + rng.integers(0, 4, size=n)) % SUBJECTS
    h["node"] = 1 + h["subject"]
    h["score"] = rng.integers(30, 300, size=n)
    h["q_lo"] = rng.integers(0, 20, size=n)
    h["q_hi"] = h["q_lo"] + rng.integers(20, 130, size=n)
    h["s_lo"] = rng.integers(0, 400, size=n) + 300 * mate
    h["s_hi"] = h["s_lo"] + 50
    h["strand"] = mate ^ (rng.random(n) < 0.1)
    return begin, np.full(npairs, 150, dtype=np.uint32), h


def measure(name, case, repeat):
    begin, offset, h = case
    as_cull = np.zeros(len(h), dtype=CULL_HIT_DTYPE)
    for f in CULL_HIT_DTYPE.names:
        as_cull[f] = h[f]
    runs = []
    cand = pairs = None
    for k in range(repeat + 1):
        c0, p0, l0 = stage_read_cull_stats(), stage_pair_join_stats(), stage_read_lca_stats()
        read_cull(begin, as_cull, 1, 50)
        t = time.perf_counter()
        cand, _, pairs = pair_join(begin, offset, h, 600, 1)
        wall = time.perf_counter() - t
        read_lca(begin[::2], cand, 10, 100)
        c1, p1, l1 = stage_read_cull_stats(), stage_pair_join_stats(), stage_read_lca_stats()
        if k:
            runs.append({"seconds_cull": c1["seconds_cull"] - c0["seconds_cull"],
                         "seconds_pair": p1["seconds_pair"] - p0["seconds_pair"],
                         "seconds_lca": l1["seconds_lca"] - l0["seconds_lca"], "wall_pair": wall,
                         "pair_launches": p1["pair_launches"] - p0["pair_launches"]})
    size = np.diff(begin[::2].astype(np.int64))
    print(json.dumps({"set": name, "pairs": int(len(offset)), "hits": int(len(h)), "largest_pair": int(size.max()),
                      "joined": int(pairs["joined"].sum()), "pairs_joined": int((pairs["joined"] > 0).sum()),
                      "runs": runs}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--large-pairs", type=int, default=4000)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    set_taxonomy_gpu(np.zeros(SUBJECTS + 1, dtype=np.uint32))   # a star: node 1 + s is subject s's leaf
    if args.pairs:
        measure("short", make_set(args.pairs, 1, 4, 20270105), args.repeat)
    if args.large_pairs:
        measure("large", make_set(args.large_pairs, 300, 512, 20270106), args.repeat)


if __name__ == "__main__":
    main()
