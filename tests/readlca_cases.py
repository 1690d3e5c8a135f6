"""Cases of the per-read taxonomic assignment (ReadLcaGpu, GhostmReadLcaHost; the
contract is above ReadLcaGpu in include/ghostm_hip.h) and an independent model
of it.

The model is brute force: the ancestor set of every vote and one counter per
node. It shares nothing with read_lca.h, which climbs level by level from the
deepest vote as the kernel does.

A case is (parent, read_begin, hits, top_pct, support_pct): the taxonomy as
parent indices, and read r's hits are hits[read_begin[r]:read_begin[r + 1]]."""
import ctypes
import random

import numpy as np

from ghostm_amd import native
from ghostm_amd import LCA_HIT_DTYPE, LCA_OUT_DTYPE

NONE = 0xFFFFFFFF
TOP = (1 << 25) - 1   # the largest score and coordinate


def hits_of(rows):
    """rows of (node, score, q_lo, q_hi)"""
    h = np.zeros(len(rows), dtype=LCA_HIT_DTYPE)
    for k, row in enumerate(rows):
        h[k] = tuple(row)
    return h


def one_read(parent, rows, top_pct=10, support_pct=100):
    return parent, np.array([0, len(rows)], dtype=np.uint32), hits_of(rows), top_pct, support_pct


def join(cases, top_pct=10, support_pct=100):
    """the reads of several cases on one taxonomy as one call's"""
    begin, parts, at = [0], [], 0
    for parent, rb, h, _, _ in cases:
        assert parent is cases[0][0]
        for r in range(len(rb) - 1):
            parts.append(h[int(rb[r]):int(rb[r + 1])])
            at += int(rb[r + 1]) - int(rb[r])
            begin.append(at)
    hits = np.concatenate(parts) if parts else np.zeros(0, dtype=LCA_HIT_DTYPE)
    return cases[0][0], np.array(begin, dtype=np.uint32), hits, top_pct, support_pct


# ------------------------------------------------------------------ the model
def depths(parent):
    """depth per node by walking every node up to the root"""
    par = [int(p) for p in parent]
    depth = [None] * len(par)
    for i in range(len(par)):
        path, n = [], i
        while depth[n] is None and par[n] != n:
            path.append(n)
            n = par[n]
        d = 0 if depth[n] is None else depth[n]
        depth[n] = d
        for k in reversed(path):
            d += 1
            depth[k] = d
    return depth


def model(parent, read_begin, hits, top_pct, support_pct, info=None):
    """Ancestor sets and counts per node. info, if a dict, gets 'failed': per
    read the number of candidates that fail the score test."""
    par = [int(p) for p in parent]
    depth = depths(parent)
    out = np.zeros(len(read_begin) - 1, dtype=LCA_OUT_DTYPE)
    failed = []
    for r in range(len(read_begin) - 1):
        h = hits[int(read_begin[r]):int(read_begin[r + 1])]
        c = h[h["score"] > 0]
        score, lo, hi = (c[f].astype(np.int64) for f in ("score", "q_lo", "q_hi"))
        shared = (lo[:, None] <= hi[None, :]) & (lo[None, :] <= hi[:, None])
        ref = np.where(shared, score[None, :], 0).max(axis=1) if len(c) else score
        passing = score * 100 >= (100 - top_pct) * ref
        failed.append(int((~passing).sum()))
        votes = [int(n) for n in c["node"][passing] if n != NONE]
        unmapped = int((c["node"][passing] == NONE).sum())
        best = int(score.max()) if len(c) else 0
        if not votes:
            out[r] = (NONE, 0, 0, 0, NONE, len(c), unmapped, best)
            continue
        count = {}
        for n in votes:
            while True:
                count[n] = count.get(n, 0) + 1
                if par[n] == n:
                    break
                n = par[n]
        thr = (support_pct * len(votes) + 99) // 100
        enough = [n for n in count if count[n] >= thr]
        node = max(enough, key=lambda n: depth[n])
        assert sum(depth[n] == depth[node] for n in enough) == 1
        lca = max((n for n in count if count[n] == len(votes)), key=lambda n: depth[n])
        out[r] = (node, depth[node], len(votes), count[node], lca, len(c), unmapped, best)
    if info is not None:
        info["failed"] = failed
    return out


# ---------------------------------------------------------------------- trees
# the small taxonomy of the shapes: two families under the root
ROOT, FAM_A, GEN_A1, GEN_A2, SP_A1A, SP_A1B, SP_A2A, FAM_B, GEN_B1, SP_B1A = range(10)
SMALL = np.array([0, 0, 1, 1, 2, 2, 3, 0, 7, 8], dtype=np.uint32)


def shuffled(parent, rnd):
    """the same tree under a random renumbering: a parent's index is not below its child's"""
    n = len(parent)
    perm = list(range(n))
    rnd.shuffle(perm)
    out = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        out[perm[i]] = perm[int(parent[i])]
    return out


def trees():
    """name -> parent array"""
    rnd = random.Random(20261201)
    t = {"single": np.zeros(1, dtype=np.uint32)}
    t["chain"] = np.array([0] + list(range(255)), dtype=np.uint32)            # depth 255
    t["star"] = np.zeros(300, dtype=np.uint32)
    t["binary"] = np.array([0] + [(k - 1) // 2 for k in range(1, 2047)], dtype=np.uint32)   # depth 10
    par = [0] + [rnd.randrange(max(0, k - 300), k) for k in range(1, 5000)]
    t["random"] = shuffled(par, rnd)
    return t


TREES = trees()
RANDOM_TREE = TREES["random"]


class Walker:
    """random nodes of a tree: by depth, below a node"""

    def __init__(self, parent):
        self.parent = [int(p) for p in parent]
        self.depth = depths(parent)
        self.children = [[] for _ in self.parent]
        for i, p in enumerate(self.parent):
            if p != i:
                self.children[p].append(i)
        self.deep = [i for i, d in enumerate(self.depth) if d >= min(4, max(self.depth))]

    def below(self, rnd, n, stop=0.3):
        while self.children[n] and rnd.random() >= stop:
            n = rnd.choice(self.children[n])
        return n

    def up(self, n, k):
        for _ in range(k):
            n = self.parent[n]
        return n


_WALKERS = {}


def walker(parent):
    key = id(parent)
    if key not in _WALKERS:
        _WALKERS[key] = Walker(parent)
    return _WALKERS[key]


def random_rows(rnd, parent, n, zero_rate=0.08):
    """n hits of one read: up to three genes (stretches of the read), each with
    its best score and hits at 55 to 100 % of it; the nodes mostly below one
    anchor, some below its ancestor two levels up, some anywhere, some none."""
    w = walker(parent)
    anchor = rnd.choice(w.deep)
    genes = [(600 * g, rnd.randrange(100, 2000)) for g in range(rnd.randrange(1, 4))]
    rows = []
    for _ in range(n):
        at, top = rnd.choice(genes)
        q_lo = at + rnd.randrange(0, 100)
        q_hi = q_lo + rnd.randrange(0, 400)
        x = rnd.random()
        node = (w.below(rnd, anchor) if x < 0.7 else w.below(rnd, w.up(anchor, 2)) if x < 0.85
                else w.below(rnd, w.up(anchor, 400)) if x < 0.93 else NONE)
        score = 0 if rnd.random() < zero_rate else max(1, top * rnd.randrange(55, 101) // 100)
        rows.append((node, score, q_lo, q_hi))
    return rows


# ---------------------------------------------------------------- small shapes
def shape_cases():
    """name -> case: the small shapes, each with what it must show."""
    c = {}
    S = SMALL
    c["no_reads"] = (S, np.zeros(1, dtype=np.uint32), hits_of([]), 10, 100)
    c["empty_read"] = (S, np.array([0, 0], dtype=np.uint32), hits_of([]), 10, 100)
    c["one_hit"] = one_read(S, [(SP_A1A, 40, 5, 60)])
    c["one_leaf"] = one_read(S, [(SP_A1A, 40 + k % 2, 5 + k, 60 + k) for k in range(5)])
    c["two_leaves_one_parent"] = one_read(S, [(SP_A1A, 40, 5, 60), (SP_A1B, 40, 5, 60)])
    c["leaf_and_ancestor"] = one_read(S, [(SP_A1A, 40, 5, 60), (GEN_A1, 40, 5, 60)])
    c["root_vote"] = one_read(S, [(SP_A1A, 40, 5, 60), (ROOT, 40, 5, 60)])
    c["all_unmapped"] = one_read(S, [(NONE, 40, 5, 60), (NONE, 39, 5, 60), (NONE, 10, 5, 60)])
    c["all_zero"] = one_read(S, [(SP_A1A, 0, 5, 60), (NONE, 0, 0, 0), (SP_B1A, 0, 7, 9)])
    between = [one_read(S, [(SP_A1A, 40, 5, 60)]), (S, np.array([0, 0], dtype=np.uint32), hits_of([]), 10, 100),
               one_read(S, [(SP_B1A, 40, 5, 60)])]
    c["empty_between"] = join(between)
    c["strong_and_weak_gene"] = one_read(S, [(SP_A1A, 1000, 0, 299), (SP_B1A, 200, 400, 699)])
    c["strong_over_weak"] = one_read(S, [(SP_A1A, 1000, 0, 299), (SP_B1A, 200, 100, 399)])
    c["touching"] = one_read(S, [(SP_A1A, 1000, 0, 99), (SP_B1A, 200, 100, 199)])
    c["one_position_shared"] = one_read(S, [(SP_A1A, 1000, 0, 100), (SP_B1A, 200, 100, 199)])
    near = [(SP_A1A, 100, 0, 99), (SP_A1B, 99, 0, 99), (SP_A2A, 100, 0, 99), (SP_B1A, 1, 0, 99)]
    c["top_pct_0"] = one_read(S, near, top_pct=0)
    c["top_pct_100"] = one_read(S, near, top_pct=100)
    three = [(SP_A1A, 50, 0, 99), (SP_A1A, 50, 0, 99), (SP_A2A, 50, 0, 99)]
    c["three_votes_67"] = one_read(S, three, support_pct=67)
    c["three_votes_66"] = one_read(S, three, support_pct=66)
    c["hundred_votes_51_49"] = one_read(S, [(SP_A1A, 50, 0, 99)] * 51 + [(SP_B1A, 50, 0, 99)] * 49, support_pct=51)
    c["hundred_votes_50_50"] = one_read(S, [(SP_A1A, 50, 0, 99)] * 50 + [(SP_B1A, 50, 0, 99)] * 50, support_pct=51)
    outlier = [(SP_A1A, 50, 0, 99)] * 9 + [(SP_B1A, 50, 0, 99)]
    c["outlier_100"] = one_read(S, outlier, support_pct=100)
    c["outlier_90"] = one_read(S, outlier, support_pct=90)
    c["top_values"] = one_read(S, [(SP_A1A, TOP, TOP - 5, TOP), (SP_A1B, TOP - TOP // 10, TOP, TOP),
                                   (SP_B1A, TOP - TOP // 10 - 1, 0, TOP)])
    return c


def expected_shapes(name, out):
    """What the small shapes are for, on the model's (or anyone's) records."""
    rec = [tuple(int(x) for x in o) for o in out]
    none = lambda cand=0, unm=0, best=0: (NONE, 0, 0, 0, NONE, cand, unm, best)   # noqa: E731
    if name == "no_reads":
        assert rec == []
    elif name == "empty_read":
        assert rec == [none()]
    elif name == "one_hit":
        assert rec == [(SP_A1A, 3, 1, 1, SP_A1A, 1, 0, 40)]
    elif name == "one_leaf":
        assert rec == [(SP_A1A, 3, 5, 5, SP_A1A, 5, 0, 41)]
    elif name == "two_leaves_one_parent":
        assert rec == [(GEN_A1, 2, 2, 2, GEN_A1, 2, 0, 40)]
    elif name == "leaf_and_ancestor":
        assert rec == [(GEN_A1, 2, 2, 2, GEN_A1, 2, 0, 40)]
    elif name == "root_vote":
        assert rec == [(ROOT, 0, 2, 2, ROOT, 2, 0, 40)]
    elif name == "all_unmapped":   # the third fails the score test: it is not counted as unmapped
        assert rec == [none(3, 2, 40)]
    elif name == "all_zero":
        assert rec == [none()]
    elif name == "empty_between":
        assert rec == [(SP_A1A, 3, 1, 1, SP_A1A, 1, 0, 40), none(), (SP_B1A, 3, 1, 1, SP_B1A, 1, 0, 40)]
    elif name == "strong_and_weak_gene":   # disjoint stretches: the weak gene votes although 200 < 90 % of 1000
        assert rec == [(ROOT, 0, 2, 2, ROOT, 2, 0, 1000)]
    elif name == "strong_over_weak":
        assert rec == [(SP_A1A, 3, 1, 1, SP_A1A, 2, 0, 1000)]
    elif name == "touching":   # q_hi + 1 == q_lo: no position shared
        assert rec == [(ROOT, 0, 2, 2, ROOT, 2, 0, 1000)]
    elif name == "one_position_shared":
        assert rec == [(SP_A1A, 3, 1, 1, SP_A1A, 2, 0, 1000)]
    elif name == "top_pct_0":   # only the best scores of the stretch
        assert rec == [(FAM_A, 1, 2, 2, FAM_A, 4, 0, 100)]
    elif name == "top_pct_100":   # every candidate
        assert rec == [(ROOT, 0, 4, 4, ROOT, 4, 0, 100)]
    elif name == "three_votes_67":   # thr 3
        assert rec == [(FAM_A, 1, 3, 3, FAM_A, 3, 0, 50)]
    elif name == "three_votes_66":   # thr 2
        assert rec == [(SP_A1A, 3, 3, 2, FAM_A, 3, 0, 50)]
    elif name == "hundred_votes_51_49":   # thr 51
        assert rec == [(SP_A1A, 3, 100, 51, ROOT, 100, 0, 50)]
    elif name == "hundred_votes_50_50":
        assert rec == [(ROOT, 0, 100, 100, ROOT, 100, 0, 50)]
    elif name == "outlier_100":
        assert rec == [(ROOT, 0, 10, 10, ROOT, 10, 0, 50)]
    elif name == "outlier_90":   # thr 9
        assert rec == [(SP_A1A, 3, 10, 9, ROOT, 10, 0, 50)]
    elif name == "top_values":   # (TOP - TOP // 10) * 100 >= 90 * TOP holds, one less does not
        assert rec == [(GEN_A1, 2, 2, 2, GEN_A1, 3, 0, TOP)]
    else:
        raise AssertionError(name)


def tree_cases():
    """name -> one call of a few reads on every tree of TREES"""
    c = {}
    for k, (name, parent) in enumerate(TREES.items()):
        rnd = random.Random(20261202 + k)
        reads = [one_read(parent, random_rows(rnd, parent, n)) for n in (1, 7, 30, 64, 90)]
        c[name] = join(reads, 10, 100 if k % 2 == 0 else 60)
    leaves = list(range(1, 300))
    c["star_leaves"] = one_read(TREES["star"], [(n, 50, 0, 9) for n in leaves[:70]])
    c["chain_ends"] = one_read(TREES["chain"], [(255, 50, 0, 9), (254, 50, 0, 9), (3, 50, 0, 9)], support_pct=60)
    return c


# ----------------------------------------------------------------- large reads
SIZES = (63, 64, 65, 1023, 1024, 1025, 2000)   # candidates: the kernel's class borders, and the device-memory tables


def sized_read(n, seed=0, parent=None):
    """One read of n candidates on the random tree, a score-0 hit after every
    ninth candidate and one in front."""
    parent = RANDOM_TREE if parent is None else parent
    rnd = random.Random(20261203 + 7 * n + seed)
    rows = []
    for k, row in enumerate(random_rows(rnd, parent, n, zero_rate=0)):
        if k % 9 == 0:
            rows.append((row[0], 0, row[2], row[3]))
        rows.append(row)
    return one_read(parent, rows, 10, 60 if n % 2 else 100)


def candidates_of(case):
    return int((case[2]["score"] > 0).sum())


def mixed_call(top_pct=10, support_pct=60):
    """every class in one call, reads without hits and without candidates between them"""
    S = RANDOM_TREE
    empty = (S, np.array([0, 0], dtype=np.uint32), hits_of([]), 10, 100)
    zeros = one_read(S, [(5, 0, 0, 9), (NONE, 0, 3, 4)])
    parts = [sized_read(5, 1), sized_read(1025, 1), sized_read(64, 1), empty, sized_read(300, 1), sized_read(65, 1),
             zeros, sized_read(1, 1), sized_read(1100, 1), empty, sized_read(700, 1), sized_read(63, 1)]
    return join(parts, top_pct, support_pct)


def random_calls(count, seed=20261204):
    """count calls of a few reads each on the random tree"""
    rnd = random.Random(seed)
    calls = []
    for _ in range(count):
        reads = [one_read(RANDOM_TREE, random_rows(rnd, RANDOM_TREE, rnd.choice((0, 1, 2, 3, 8, 20, 40, 70))))
                 for _ in range(rnd.randrange(1, 5))]
        calls.append(join(reads, rnd.choice((0, 10, 10, 30, 100)), rnd.choice((51, 60, 60, 90, 100))))
    return calls


def assert_same(got, want, what):
    assert got.dtype == want.dtype == LCA_OUT_DTYPE and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


# ------------------------------------------------------------------- refusals
def refusals():
    """(reason, read_begin, hits, top_pct, support_pct) on SMALL: every reason of the contract but "taxonomy" """
    h = hits_of([(SP_A1A, 50, 0, 99), (SP_B1A, 40, 10, 20), (NONE, 30, 100, 120)])

    def changed(k, field, value):
        g = h.copy()
        g[field][k] = value
        return g

    rb = np.array([0, 2, 3], dtype=np.uint32)
    many = np.zeros(16385, dtype=LCA_HIT_DTYPE)
    many["score"] = 1
    return [
        ("reads", np.array([0, 3, 2], dtype=np.uint32), h, 10, 100),
        ("reads", np.array([0, 2, 4], dtype=np.uint32), h, 10, 100),
        ("reads", np.array([0, 16385], dtype=np.uint32), many, 10, 100),
        ("range", rb, changed(1, "q_lo", 21), 10, 100),
        ("bounds", rb, changed(2, "q_hi", TOP + 1), 10, 100),
        ("bounds", rb, changed(0, "score", TOP + 1), 10, 100),
        ("node", rb, changed(0, "node", len(SMALL)), 10, 100),
        ("node", rb, changed(2, "node", NONE - 1), 10, 100),
        ("param", rb, h, 101, 100),
        ("param", rb, h, 10, 50),
        ("param", rb, h, 10, 101),
    ]


def raw_call(fn, parent, rb, h, top_pct, support_pct, out):
    """the entry point itself; None for a null pointer. parent None: ReadLcaGpu's arguments."""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    tax = () if parent is None else (len(parent), parent.ctypes.data_as(u32p))
    return fn(*tax, 0 if rb is None else len(rb) - 1, None if rb is None else rb.ctypes.data_as(u32p),
              0 if h is None else len(h), None if h is None else h.ctypes.data_as(ctypes.POINTER(native.GhostmLcaHit)),
              top_pct, support_pct, None if out is None else out.ctypes.data_as(ctypes.POINTER(native.GhostmLcaOut)))


def check_refusals(fn_name, with_parent):
    """Every reason on one entry point; the outputs keep their bytes. For
    ReadLcaGpu (with_parent False) SMALL is resident."""
    fn = getattr(native.load(), fn_name)
    parent = SMALL if with_parent else None
    for reason, rb, h, top_pct, support_pct in refusals():
        out = np.full(8 * len(rb), 0xC3C3C3C3, dtype=np.uint32).view(LCA_OUT_DTYPE)
        assert raw_call(fn, parent, rb, h, top_pct, support_pct, out) == 1, reason
        msg = native.last_error()
        assert msg.startswith(fn_name + ": ") and (reason + ": ") in msg, (reason, msg)
        assert (out.view(np.uint32) == 0xC3C3C3C3).all(), reason
    _, rb, h, top_pct, support_pct = shape_cases()["strong_and_weak_gene"]
    out = np.zeros(1, dtype=LCA_OUT_DTYPE)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    tax = () if parent is None else (len(parent), parent.ctypes.data_as(u32p))
    hp, op = ctypes.POINTER(native.GhostmLcaHit), ctypes.POINTER(native.GhostmLcaOut)
    for null in ("read_begin", "hit", "out"):
        rc = fn(*tax, len(rb) - 1, None if null == "read_begin" else rb.ctypes.data_as(u32p), len(h),
                None if null == "hit" else h.ctypes.data_as(hp), top_pct, support_pct,
                None if null == "out" else out.ctypes.data_as(op))
        assert rc == 1 and "null: " in native.last_error(), (null, native.last_error())
    assert not out.view(np.uint32).any()
    assert fn(*tax, 0, None, 0, None, 10, 100, None) == 0   # nothing to do needs no pointer


BAD_TREES = {   # name -> (parent, the node the message names or None)
    "two_roots": (np.array([0, 1, 0], dtype=np.uint32), 1),
    "no_root": (np.array([1, 0], dtype=np.uint32), None),
    "three_cycle": (np.array([0, 2, 3, 1, 0], dtype=np.uint32), 1),
    "depth_256": (np.array([0] + list(range(256)), dtype=np.uint32), 256),
    "parent_out_of_range": (np.array([0, 0, 3], dtype=np.uint32), 2),
}
