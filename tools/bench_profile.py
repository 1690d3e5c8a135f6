"""Time a sample's taxon profile (the k_taxon_* kernels; -y 24 / -y 25,
Session.taxon_profile) at the stage level, beside the host model and the
per-read assignment that produces its input, at two taxonomy sizes.

One synthetic tree: the first 2^16 nodes a seeded random tree about 30 levels
deep, every further node a child of one of those, so that a tree of --nodes
nodes is a prefix of a larger one and the same reads are valid on both. The
reads (--reads, default 1 M) fall on --distinct nodes (default 4000) of the
first 2^16 with a skewed distribution, one in twenty without a taxon. Per tree
size: SetTaxonomyGpu's wall time (it allocates and zeroes the count arrays),
then --repeat times, after one run left out, ReadLcaGpu on three equal hits per
read (seconds_lca, wall), TaxonProfileGpu on the nodes it assigned
(seconds_profile, wall of the whole call, launches) and GhostmTaxonProfileHost
on the same input (wall). The device times at the two sizes are the evidence
that a call's work follows the nodes the sample touches and not the
taxonomy's. Prints one JSON line.

    python tools/bench_profile.py --reads 1000000 --nodes 65536 16777216 --repeat 5
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

from ghostm_amd import (LCA_HIT_DTYPE, native, read_lca, set_taxonomy_gpu, stage_read_lca_stats,  # noqa: E402
                        stage_taxon_profile_stats, taxon_profile, taxon_profile_host, taxonomy_depths)

CORE = 1 << 16
NONE = 0xFFFFFFFF


def synthetic_tree(nnodes: int, seed: int = 20270105, depth: int = 20) -> np.ndarray:
    """parent indices: node k < 2^16 under a random node of the window before
    it, node k >= 2^16 under a random node of the first 2^16"""
    rng = np.random.default_rng(seed)
    core = min(nnodes, CORE)
    k = np.arange(core, dtype=np.int64)
    window = np.minimum(k, max(2, 2 * core // depth))
    parent = k - 1 - (rng.random(core) * window).astype(np.int64)
    parent[0] = 0
    if nnodes > core:   # drawn after the core, so the core does not depend on nnodes
        parent = np.concatenate([parent, np.random.default_rng(seed + 1).integers(0, core, nnodes - core)])
    return parent.astype(np.uint32)


def synthetic_reads(nreads: int, distinct: int, seed: int = 20270106) -> np.ndarray:
    rng = np.random.default_rng(seed)
    nodes = rng.choice(np.arange(1, CORE), size=distinct, replace=False).astype(np.uint32)
    weight = 1.0 / np.arange(1, distinct + 1)   # a few abundant taxa, a long tail
    node = nodes[rng.choice(distinct, size=nreads, p=weight / weight.sum())]
    node[rng.random(nreads) < 0.05] = NONE
    return node


def measure(parent, node, min_reads, repeat):
    t = time.perf_counter()
    set_taxonomy_gpu(parent)
    wall_set = time.perf_counter() - t
    nreads = len(node)
    hits = np.zeros(3 * nreads, dtype=LCA_HIT_DTYPE)
    hits["node"] = np.repeat(node, 3)
    hits["score"] = 100
    hits["q_hi"] = 99
    begin = np.arange(0, 3 * nreads + 1, 3, dtype=np.uint32)
    need = len(taxon_profile(node, min_reads, with_final=False)[0])   # the count query, then the records
    runs = []
    for k in range(repeat + 1):
        l0 = stage_read_lca_stats()
        t = time.perf_counter()
        lca = read_lca(begin, hits)
        wall_lca = time.perf_counter() - t
        l1 = stage_read_lca_stats()
        assigned = np.ascontiguousarray(lca["node"])
        assert np.array_equal(assigned, node)
        p0 = stage_taxon_profile_stats()
        t = time.perf_counter()
        got = taxon_profile(assigned, min_reads, cap=need, with_final=True)
        wall = time.perf_counter() - t
        p1 = stage_taxon_profile_stats()
        t = time.perf_counter()
        want = taxon_profile_host(parent, assigned, min_reads, cap=need, with_final=True)
        wall_host = time.perf_counter() - t
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        if not k:
            continue
        runs.append(dict(seconds_profile=p1["seconds_profile"] - p0["seconds_profile"], wall_profile=wall,
                         profile_launches=p1["profile_launches"] - p0["profile_launches"], wall_host=wall_host,
                         seconds_lca=l1["seconds_lca"] - l0["seconds_lca"], wall_lca=wall_lca))
    return dict(nodes=int(len(parent)), tree_depth=int(taxonomy_depths(parent).max()), wall_set_taxonomy=wall_set,
                records=int(len(got[0])), summary=got[2], runs=runs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--distinct", type=int, default=4000)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1 << 16, 1 << 24])
    ap.add_argument("--min-reads", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    node = synthetic_reads(args.reads, args.distinct)
    out = {"reads": args.reads, "distinct_nodes": int(len(np.unique(node[node != NONE]))), "min_reads": args.min_reads,
           "batch_reads": os.environ.get("GHOSTM_PROFILE_BATCH_READS", "no limit"), "trees": []}
    for nnodes in args.nodes:
        if nnodes < CORE:
            raise SystemExit("--nodes: at least 65536 (the reads fall on the first 2^16 nodes)")
        out["trees"].append(measure(synthetic_tree(nnodes), node, args.min_reads, args.repeat))
    native.load().FreeGpu()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
