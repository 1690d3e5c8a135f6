"""Cases of a sample's taxon profile (TaxonProfileGpu, GhostmTaxonProfileHost; the
contract is above TaxonProfileGpu in include/ghostm_hip.h), an independent
model of it and of the -y 24 / -y 25 report.

The model is written from the definitions: per read the list of nodes from its
node to the root, a dictionary of clade counts, the first node of that list at
or over the floor. It shares nothing with taxon_profile.h (dense arrays, a climb
per distinct node) or the kernels (lists of touched nodes).

A case is (parent, node, min_reads): the taxonomy as parent indices, node[r] the
read's node index or NONE."""
import ctypes
import random

import numpy as np

import readlca_cases as lc
from ghostm_amd import TAXON_COUNT_DTYPE, native

NONE = 0xFFFFFFFF
TREES = lc.TREES
SMALL = lc.SMALL
BLOCK = 256   # the kernels' workgroup: one lane per read or per node


# ------------------------------------------------------------------ the model
def path(par, n):
    out = [n]
    while par[n] != n:
        n = par[n]
        out.append(n)
    return out


def model(parent, node, min_reads):
    """(records, final nodes, summary) from the definitions"""
    par = [int(p) for p in parent]
    node = [int(n) for n in node]
    paths = {n: path(par, n) for n in set(node) if n != NONE}
    direct, clade = {}, {}
    for n in node:
        if n == NONE:
            continue
        direct[n] = direct.get(n, 0) + 1
        for a in paths[n]:
            clade[a] = clade.get(a, 0) + 1
    final = []
    for n in node:
        f = NONE
        if n != NONE:
            f = next((a for a in paths[n] if clade[a] >= min_reads), NONE)
        final.append(f)
    kept = {}
    for f in final:
        if f != NONE:
            kept[f] = kept.get(f, 0) + 1
    rec = np.zeros(len(clade), dtype=TAXON_COUNT_DTYPE)
    for k, n in enumerate(sorted(clade)):
        rec[k] = (n, clade[n], direct.get(n, 0), kept.get(n, 0))
    summary = dict(reads=len(node), classified=sum(n != NONE for n in node), kept=sum(f != NONE for f in final),
                   moved=sum(f != NONE and f != n for n, f in zip(node, final)), nodes=len(clade),
                   nodes_kept=sum(c >= min_reads for c in clade.values()))
    return rec, np.array(final, dtype=np.uint32), summary


def check_invariants(parent, rec, final, summary, min_reads):
    """what follows from the definitions, on anyone's result"""
    s = summary
    assert int(rec["direct_reads"].sum()) == s["classified"] and int(rec["kept_reads"].sum()) == s["kept"]
    assert s["kept"] == (s["classified"] if s["classified"] >= min_reads else 0)
    assert s["nodes"] == len(rec) and (np.diff(rec["node"].astype(np.int64)) > 0).all()
    assert (rec["clade_reads"] > 0).all() and (rec["kept_reads"][rec["clade_reads"] < min_reads] == 0).all()
    assert s["nodes_kept"] == int((rec["clade_reads"] >= min_reads).sum())
    assert int((final != NONE).sum()) == s["kept"] and len(final) == s["reads"]
    if s["classified"]:
        root = next(i for i, p in enumerate(parent) if int(p) == i)
        at = rec[rec["node"] == root]
        assert len(at) == 1 and at["clade_reads"][0] == s["classified"]
    by_node = {int(r["node"]): int(r["clade_reads"]) for r in rec}
    for r in rec:   # clade never shrinks towards the root
        assert by_node[int(parent[r["node"]])] >= r["clade_reads"]


def assert_same(got, want, what):
    """(records, final, summary) against (records, final, summary)"""
    (grec, gfin, gsum), (wrec, wfin, wsum) = got, want
    assert grec.dtype == wrec.dtype == TAXON_COUNT_DTYPE, what
    if len(grec) != len(wrec) or not np.array_equal(grec, wrec):
        n = min(len(grec), len(wrec))
        bad = np.flatnonzero(grec[:n] != wrec[:n])
        first = (grec[bad[0]], wrec[bad[0]]) if len(bad) else "a length"
        raise AssertionError(f"{what}: {len(grec)} records against {len(wrec)}, {len(bad)} differ, first {first}")
    if gfin is not None and wfin is not None:
        assert gfin.dtype == np.uint32 and np.array_equal(gfin, wfin), (what, "final")
    assert gsum == wsum, (what, gsum, wsum)


# ----------------------------------------------------------------- the report
def percent(part, total):
    h = (part * 10000 + total // 2) // total
    return "%d.%02d" % (h // 100, h % 100)


def report(parent, taxid, rec, min_reads, total):
    """the text of -y 24 / -y 25 from a profile's records: recursive, children sorted per node"""
    if total == 0:
        return b""
    par = [int(p) for p in parent]
    depth = lc.depths(parent)
    rows = {int(r["node"]): r for r in rec if r["clade_reads"] >= min_reads}
    kept = int(rec["kept_reads"].sum())
    lines = []
    if total > kept:
        u = total - kept
        lines.append("%s\t%d\t%d\t%d\t0\t0\t0" % (percent(u, total), u, u, u))
    children = {}
    root = None
    for n in rows:
        if par[n] == n:
            root = n
        else:
            children.setdefault(par[n], []).append(n)

    def walk(n):
        r = rows[n]
        lines.append("%s\t%d\t%d\t%d\t%d\t%d\t%d" % (percent(int(r["clade_reads"]), total), r["clade_reads"], r["kept_reads"],
                                                     r["direct_reads"], depth[n], taxid[n], taxid[par[n]]))
        for c in sorted(children.get(n, []), key=lambda c: (-int(rows[c]["clade_reads"]), int(taxid[c]))):
            walk(c)

    if root is not None:
        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
        walk(root)
    return ("\n".join(lines) + "\n").encode() if lines else b""


# the hand-written sample on SMALL: two reads without a taxon, a tie between the
# families (broken by taxid: FAM_B's is the smaller), clades under a floor of 2
SMALL_TAXID = np.array([1, 10, 20, 21, 30, 31, 32, 5, 22, 33], dtype=np.uint32)
SMALL_NODES = np.array([NONE, lc.SP_A1A, lc.SP_B1A, lc.SP_A1A, lc.SP_A1B, lc.SP_B1A, lc.ROOT, lc.SP_A2A, lc.SP_B1A, NONE,
                        lc.SP_A1A, lc.SP_B1A, lc.SP_B1A], dtype=np.uint32)
SMALL_MIN = 2
SMALL_REPORT = (b"15.38\t2\t2\t2\t0\t0\t0\n"       # 2 of 13
                b"84.62\t11\t1\t1\t0\t1\t1\n"      # the root: 84.615 rounds up
                b"38.46\t5\t0\t0\t1\t5\t1\n"       # FAM_B before FAM_A: 5 reads each, taxid 5 < 10
                b"38.46\t5\t0\t0\t2\t22\t5\n"
                b"38.46\t5\t5\t5\t3\t33\t22\n"
                b"38.46\t5\t1\t0\t1\t10\t1\n"      # FAM_A keeps SP_A2A's read: GEN_A2 and SP_A2A are under the floor
                b"30.77\t4\t1\t0\t2\t20\t10\n"     # GEN_A1 keeps SP_A1B's
                b"23.08\t3\t3\t3\t3\t30\t20\n")
SMALL_RECORDS = [(0, 11, 1, 1), (1, 5, 0, 1), (2, 4, 0, 1), (3, 1, 0, 0), (4, 3, 3, 3), (5, 1, 1, 0), (6, 1, 1, 0),
                 (7, 5, 0, 0), (8, 5, 0, 0), (9, 5, 5, 5)]


# ---------------------------------------------------------------------- cases
def sample(parent, n, seed, none_rate=0.1, hot=8):
    """n reads on a tree: most below a few hot anchors, some anywhere, some without a taxon"""
    rnd = random.Random(20270101 + seed)
    w = lc.walker(parent)
    anchors = [rnd.choice(w.deep) for _ in range(hot)]
    out = []
    for _ in range(n):
        x = rnd.random()
        if x < none_rate:
            out.append(NONE)
        elif x < 0.8:
            out.append(w.below(rnd, rnd.choice(anchors)))
        else:
            out.append(rnd.randrange(len(parent)))
    return np.array(out, dtype=np.uint32)


COUNTS = (0, 1, 63, 64, 65, 257)   # the wave's and the workgroup's borders; 257 is one above the workgroup


def count_cases():
    """every read count with all reads on one node, each on its own node, all without a taxon"""
    tree = TREES["random"]
    c = {}
    for n in COUNTS:
        c[f"one_node_{n}"] = (tree, np.full(n, 4321, dtype=np.uint32), 1)
        c[f"own_node_{n}"] = (tree, (np.arange(n, dtype=np.uint32) * 19 + 7) % len(tree), 2)
        c[f"none_{n}"] = (tree, np.full(n, NONE, dtype=np.uint32), 1)
    return c


def tree_cases():
    c = {}
    c["single"] = (TREES["single"], np.zeros(70, dtype=np.uint32), 1)
    c["chain_one_leaf"] = (TREES["chain"], np.array([255], dtype=np.uint32), 1)          # 256 records
    c["chain_contention"] = (TREES["chain"], np.full(100000, 255, dtype=np.uint32), 3)   # one path, 1563 waves
    c["chain_spread"] = (TREES["chain"], np.arange(256, dtype=np.uint32).repeat(2), 300)
    c["star"] = (TREES["star"], np.arange(1, 300, dtype=np.uint32), 2)                   # 299 leaves, all direct
    c["binary_full"] = (TREES["binary"], np.arange(2047, dtype=np.uint32), 4)            # the touched list is the tree
    c["random"] = (TREES["random"], sample(TREES["random"], 3000, 1), 5)
    c["small"] = (SMALL, SMALL_NODES, SMALL_MIN)
    return c


def floor_cases():
    """min_reads at 1, 2, a clade count exactly and one more, classified and one more"""
    tree = TREES["random"]
    node = sample(tree, 2000, 2)
    rec, _, summary = model(tree, node, 1)
    between = sorted({int(x) for x in rec["clade_reads"] if 2 < x < summary["classified"]})
    assert len(between) >= 3
    mid = between[len(between) // 2]   # a count some clade has exactly
    floors = (1, 2, mid, mid + 1, summary["classified"], summary["classified"] + 1)
    return {f"floor_{m}": (tree, node, m) for m in floors}


def random_calls(count=150, seed=20270102):
    rnd = random.Random(seed)
    calls = []
    for k in range(count):
        n = rnd.choice((0, 1, 2, 5, 30, 64, 100, 200, 300))
        calls.append((TREES["random"], sample(TREES["random"], n, 100 + k, none_rate=rnd.choice((0, 0.1, 0.5))),
                      rnd.choice((1, 1, 2, 3, 5, 20))))
    return calls


def stage_cases():
    c = {}
    c.update(count_cases())
    c.update(tree_cases())
    c.update(floor_cases())
    return c


# ------------------------------------------------------------------- refusals
def raw_call(fn, parent, node, min_reads, cap, out, nout, final, summary):
    """the entry point itself; None for a null pointer. parent None: TaxonProfileGpu's arguments."""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    tax = () if parent is None else (len(parent), parent.ctypes.data_as(u32p))
    return fn(*tax, 0 if node is None else len(node), None if node is None else node.ctypes.data_as(u32p), min_reads, cap,
              None if out is None else out.ctypes.data_as(ctypes.POINTER(native.GhostmTaxonCount)),
              None if nout is None else ctypes.byref(nout), None if final is None else final.ctypes.data_as(u32p),
              None if summary is None else ctypes.byref(summary))


POISON = 0xC3C3C3C3


def check_refusals(fn_name, with_parent):
    """Every reason but "taxonomy" on one entry point, on SMALL (resident for
    TaxonProfileGpu); every output keeps its bytes."""
    fn = getattr(native.load(), fn_name)
    parent = SMALL if with_parent else None
    good = SMALL_NODES
    bad_node = good.copy()
    bad_node[5] = len(SMALL)
    almost_none = good.copy()
    almost_none[7] = NONE - 1
    need = len(SMALL_RECORDS)
    for reason, node, min_reads, cap, null in (("param: ", good, 0, 16, None), ("null: node", good, 1, 16, "node"),
                                               ("null: nout", good, 1, 16, "nout"), ("null: out", good, 1, 16, "out"),
                                               ("node: read 5:", bad_node, 1, 16, None),
                                               ("node: read 7:", almost_none, 1, 16, None),
                                               (f"cap: {need} ", good, 1, need - 1, None),
                                               (f"cap: {need} ", good, 1, 0, "keep_out")):
        out = np.full(4 * 16, POISON, dtype=np.uint32).view(TAXON_COUNT_DTYPE)
        final = np.full(len(good), POISON, dtype=np.uint32)
        nout = ctypes.c_size_t(POISON)
        summary = native.GhostmTaxonSummary(*([POISON] * 6))
        rc = fn(*(() if parent is None else (len(parent), parent.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))),
                len(node), None if null == "node" else node.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), min_reads, cap,
                None if null == "out" else out.ctypes.data_as(ctypes.POINTER(native.GhostmTaxonCount)),
                None if null == "nout" else ctypes.byref(nout), final.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                ctypes.byref(summary))
        msg = native.last_error()
        assert rc == 1 and msg.startswith(fn_name + ": ") and reason in msg, (reason, msg)
        assert (out.view(np.uint32) == POISON).all() and (final == POISON).all() and nout.value == POISON, reason
        assert all(getattr(summary, n) == POISON for n, _ in summary._fields_), reason
    # the count query: cap 0 and no out sets nout alone
    final = np.full(len(good), POISON, dtype=np.uint32)
    nout = ctypes.c_size_t(POISON)
    summary = native.GhostmTaxonSummary(*([POISON] * 6))
    assert raw_call(fn, parent, good, SMALL_MIN, 0, None, nout, final, summary) == 0
    assert nout.value == need and (final == POISON).all() and summary.reads == POISON
    # nothing to do needs no pointer but nout
    nout = ctypes.c_size_t(POISON)
    assert raw_call(fn, parent, None, 1, 0, None, nout, None, None) == 0 and nout.value == 0
