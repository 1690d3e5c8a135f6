"""Cases of the read-level cull (ReadCullGpu, GhostmReadCullHost; the contract is
above ReadCullGpu in include/ghostm_hip.h) and an independent model of it.

The model is brute force: a plain loop over the hits in sorted order and one
counter per position of the read. It shares nothing with read_cull.h, which
works on segments between sorted endpoints as the kernel does.

A case is (read_begin, hits, top_k, cover_pct): read r's hits are
hits[read_begin[r]:read_begin[r + 1]]."""
import ctypes
import random

import numpy as np

from ghostm_amd import native
from ghostm_amd import CULL_CULLED, CULL_DUP, CULL_EMPTY, CULL_HIT_DTYPE, CULL_KEPT, CULL_OUT_DTYPE

NONE = 0xFFFFFFFF
TOP = (1 << 25) - 1   # the largest coordinate


def hits_of(rows):
    """rows of (subject, score, q_lo, q_hi, s_lo, s_hi)"""
    h = np.zeros(len(rows), dtype=CULL_HIT_DTYPE)
    for k, row in enumerate(rows):
        h[k] = tuple(row)
    return h


def one_read(rows, top_k=1, cover_pct=50):
    return np.array([0, len(rows)], dtype=np.uint32), hits_of(rows), top_k, cover_pct


def join(cases, top_k=1, cover_pct=50):
    """the reads of several cases as one call's"""
    begin, parts, at = [0], [], 0
    for rb, h, _, _ in cases:
        for r in range(len(rb) - 1):
            n = int(rb[r + 1]) - int(rb[r])
            parts.append(h[int(rb[r]):int(rb[r + 1])])
            at += n
            begin.append(at)
    hits = np.concatenate(parts) if parts else np.zeros(0, dtype=CULL_HIT_DTYPE)
    return np.array(begin, dtype=np.uint32), hits, top_k, cover_pct


# ------------------------------------------------------------------ the model
def model(read_begin, hits, top_k, cover_pct):
    """Per-position counters and a sorted loop."""
    out = np.zeros(len(hits), dtype=CULL_OUT_DTYPE)
    for r in range(len(read_begin) - 1):
        b, e = int(read_begin[r]), int(read_begin[r + 1])
        if e == b:
            continue
        h = hits[b:e]
        base = int(h["q_lo"].min())
        depth = np.zeros(int(h["q_hi"].max()) - base + 1, dtype=np.int64)
        ranking = sorted(range(e - b), key=lambda i: (-int(h["score"][i]), i))
        kept = []
        for place, i in enumerate(ranking):
            sub, score, q_lo, q_hi, s_lo, s_hi = (int(x) for x in h[i])
            if score == 0:
                out[b + i] = (place, CULL_EMPTY, NONE, 0)
                continue
            dup = None
            for k in kept:
                o = h[k]
                if (int(o["subject"]) == sub and int(o["q_lo"]) <= q_hi and q_lo <= int(o["q_hi"])
                        and int(o["s_lo"]) <= s_hi and s_lo <= int(o["s_hi"])):
                    dup = k
                    break
            if dup is not None:
                out[b + i] = (place, CULL_DUP, NONE, b + dup)
                continue
            d = int((depth[q_lo - base:q_hi - base + 1] >= top_k).sum())
            if d * 100 >= cover_pct * (q_hi - q_lo + 1):
                out[b + i] = (place, CULL_CULLED, NONE, d)
                continue
            out[b + i] = (place, CULL_KEPT, len(kept), d)
            kept.append(i)
            depth[q_lo - base:q_hi - base + 1] += 1
    return out


# ---------------------------------------------------------------- small shapes
def nested_stack():
    """five nested hits on five subjects, the widest first in rank"""
    return [(k, 100 - k, 10 * k, 100 - 10 * k, 0, 50) for k in range(5)]


def half_covered():
    """the second hit's 100 positions: exactly 50 under the first"""
    return [(0, 90, 0, 49, 0, 49), (1, 80, 0, 99, 0, 99)]


def shape_cases():
    """name -> case: the small shapes, each with what it must show."""
    c = {}
    c["no_reads"] = (np.zeros(1, dtype=np.uint32), hits_of([]), 1, 50)
    c["empty_read"] = (np.array([0, 0], dtype=np.uint32), hits_of([]), 1, 50)
    c["one_hit"] = one_read([(3, 40, 5, 60, 7, 62)])
    c["identical_pair"] = one_read([(3, 40, 5, 60, 7, 62), (3, 40, 5, 60, 7, 62)])
    c["equal_scores"] = one_read([(1, 50, 0, 99, 0, 99), (2, 50, 0, 99, 0, 99), (3, 50, 200, 299, 0, 99)])
    c["touching"] = one_read([(1, 50, 0, 99, 0, 99), (1, 40, 100, 199, 100, 199)])
    c["one_position_overlap"] = one_read([(1, 50, 0, 100, 0, 100), (1, 40, 100, 199, 100, 199),
                                          (2, 30, 100, 199, 0, 99)])
    c["nested"] = one_read([(1, 50, 0, 199, 0, 199), (2, 40, 50, 99, 0, 49), (3, 30, 150, 260, 0, 110)])
    c["same_subject_disjoint_s"] = one_read([(1, 50, 0, 99, 0, 99), (1, 40, 300, 399, 500, 599),
                                             (1, 30, 310, 390, 100, 180)], cover_pct=100)
    c["zero_in_the_middle"] = one_read([(1, 50, 0, 99, 0, 99), (2, 0, 0, 500, 0, 500), (3, 40, 200, 299, 0, 99),
                                        (4, 0, 0, 10, 0, 10), (5, 45, 400, 450, 0, 50)])
    for k in (1, 2, 3):
        c[f"stack_top_k_{k}"] = one_read(nested_stack(), top_k=k, cover_pct=100)
    for pct in (1, 50, 100):
        c[f"half_cover_pct_{pct}"] = one_read(half_covered(), cover_pct=pct)
    top = [(1, 9, TOP - 150, TOP, TOP - 150, TOP), (1, 8, TOP - 100, TOP - 10, TOP - 100, TOP - 10),
           (2, 7, TOP - 120, TOP, 0, 120), (3, 6, TOP, TOP, TOP, TOP), (4, 5, TOP - 400, TOP - 100, 0, 300)]
    c["top_coordinates"] = one_read(top)
    return c


def expected_shapes(name, out):
    """What the small shapes are for, on the model's (or anyone's) records."""
    st = out["status"].tolist()
    if name == "one_hit":
        assert out[0].tolist() == (0, CULL_KEPT, 0, 0)
    elif name == "identical_pair":
        assert out[0].tolist() == (0, CULL_KEPT, 0, 0) and out[1].tolist() == (1, CULL_DUP, NONE, 0)
    elif name == "equal_scores":   # the index breaks the tie; the second is fully covered by the first
        assert out["order"].tolist() == [0, 1, 2] and st == [CULL_KEPT, CULL_CULLED, CULL_KEPT]
        assert out["kept_rank"].tolist() == [0, NONE, 1]
    elif name == "touching":   # q_hi + 1 == the next q_lo: neither a duplicate nor covered
        assert st == [CULL_KEPT, CULL_KEPT] and out["detail"].tolist() == [0, 0]
    elif name == "one_position_overlap":
        assert st == [CULL_KEPT, CULL_DUP, CULL_KEPT] and out["detail"].tolist() == [0, 0, 1]
    elif name == "nested":
        assert st == [CULL_KEPT, CULL_CULLED, CULL_KEPT] and out["detail"].tolist() == [0, 50, 50]
    elif name == "same_subject_disjoint_s":   # q meets, s does not: no duplicate; then covered in full
        assert st == [CULL_KEPT, CULL_KEPT, CULL_CULLED] and out["detail"][2] == 81
    elif name == "zero_in_the_middle":
        assert st == [CULL_KEPT, CULL_EMPTY, CULL_KEPT, CULL_EMPTY, CULL_KEPT]
        assert out["order"].tolist() == [0, 3, 2, 4, 1] and out["kept_rank"].tolist() == [0, NONE, 2, NONE, 1]
    elif name.startswith("stack_top_k_"):   # cover_pct 100: hit k is culled once k >= top_k hits hold it whole
        k = int(name[-1])
        assert st == [CULL_KEPT] * k + [CULL_CULLED] * (5 - k)
    elif name.startswith("half_cover_pct_"):   # d * 100 == 50 * len: the equality is culled
        pct = int(name.rsplit("_", 1)[1])
        assert out["detail"][1] == 50 and st[1] == (CULL_CULLED if pct <= 50 else CULL_KEPT)
    elif name == "top_coordinates":
        assert st == [CULL_KEPT, CULL_DUP, CULL_CULLED, CULL_CULLED, CULL_KEPT]
        assert out["detail"].tolist() == [0, 0, 121, 1, 51]


# ----------------------------------------------------------------- large reads
SIZES = (63, 64, 65, 256, 257, 1024, 1025)   # the kernel's class borders, and the device-memory tables


def random_rows(rnd, n, span, subjects, zero_rate=0.05, score_top=60):
    """n hits with coordinates below span: short and long ranges, few subjects
    and few scores, so that ties, duplicates and covered hits all occur."""
    rows = []
    for _ in range(n):
        length = rnd.choice((1, 2, 5, 30, 100, span // 2))
        q_lo = rnd.randrange(0, span - 1)
        q_hi = min(span - 1, q_lo + rnd.randrange(0, length))
        s_lo = rnd.randrange(0, span - 1)
        s_hi = min(span - 1, s_lo + (q_hi - q_lo) + rnd.randrange(0, 3))
        score = 0 if rnd.random() < zero_rate else rnd.randrange(1, score_top)
        rows.append((rnd.randrange(subjects), score, q_lo, q_hi, s_lo, s_hi))
    return rows


def sized_read(n, seed=0):
    """One read of n hits that keeps many: mostly short ranges over a long read,
    so the kept list and the segment table both grow with n."""
    rnd = random.Random(20261120 + 7 * n + seed)
    rows = random_rows(rnd, n, 40 * n + 50, 4, score_top=4 * n)
    return one_read(rows, top_k=1 + n % 3, cover_pct=50)


def mixed_call(top_k=2, cover_pct=40):
    """every class in one call, reads without hits between them"""
    parts = [sized_read(n, seed=1) for n in (5, 1025, 64, 0, 300, 65, 1, 1100, 0, 700, 63)]
    parts += [shape_cases()[k] for k in ("nested", "zero_in_the_middle", "empty_read", "identical_pair")]
    return join(parts, top_k, cover_pct)


def random_calls(count, seed=20261121):
    """count calls of a few reads each, coordinates below 2000"""
    rnd = random.Random(seed)
    calls = []
    for _ in range(count):
        reads = []
        for _ in range(rnd.randrange(1, 5)):
            n = rnd.choice((0, 1, 2, 3, 8, 20, 40, 70))
            reads.append(one_read(random_rows(rnd, n, rnd.choice((3, 50, 2000)), rnd.choice((1, 3)))))
        calls.append(join(reads, rnd.choice((1, 1, 2, 3, 255)), rnd.choice((1, 30, 50, 80, 100))))
    return calls


def assert_same(got, want, what):
    assert got.dtype == want.dtype == CULL_OUT_DTYPE and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


# ------------------------------------------------------------------- refusals
def refusals():
    """(reason, read_begin, hits, top_k, cover_pct): every reason of the contract"""
    rows = [(1, 50, 0, 99, 0, 99), (2, 40, 10, 20, 5, 15), (3, 30, 100, 120, 0, 20)]
    h = hits_of(rows)

    def changed(k, field, value):
        g = h.copy()
        g[field][k] = value
        return g

    rb = np.array([0, 2, 3], dtype=np.uint32)
    return [
        ("reads", np.array([0, 3, 2], dtype=np.uint32), h, 1, 50),
        ("reads", np.array([0, 2, 4], dtype=np.uint32), h, 1, 50),
        ("range", rb, changed(1, "q_lo", 21), 1, 50),
        ("range", rb, changed(0, "s_lo", 100), 1, 50),
        ("bounds", rb, changed(2, "q_hi", TOP + 1), 1, 50),
        ("bounds", rb, changed(0, "s_hi", TOP + 1), 1, 50),
        ("param", rb, h, 0, 50),
        ("param", rb, h, 256, 50),
        ("param", rb, h, 1, 0),
        ("param", rb, h, 1, 101),
    ]


def raw_call(fn, rb, h, top_k, pct, out):
    """the entry point itself; None for a null pointer"""
    u32p = ctypes.POINTER(ctypes.c_uint32)
    return fn(0 if rb is None else len(rb) - 1, None if rb is None else rb.ctypes.data_as(u32p),
              0 if h is None else len(h), None if h is None else h.ctypes.data_as(ctypes.POINTER(native.GhostmCullHit)),
              top_k, pct, None if out is None else out.ctypes.data_as(ctypes.POINTER(native.GhostmCullOut)))


def check_refusals(fn_name):
    """Every reason on one entry point; the outputs keep their bytes."""
    fn = getattr(native.load(), fn_name)
    for reason, rb, h, top_k, pct in refusals():
        out = np.full(4 * len(h), 0xC3C3C3C3, dtype=np.uint32).view(CULL_OUT_DTYPE)
        assert raw_call(fn, rb, h, top_k, pct, out) == 1, reason
        msg = native.last_error()
        assert msg.startswith(fn_name + ": ") and (reason + ": ") in msg, (reason, msg)
        assert (out.view(np.uint32) == 0xC3C3C3C3).all(), reason
    rb, h, top_k, pct = shape_cases()["nested"]
    out = np.zeros(len(h), dtype=CULL_OUT_DTYPE)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    hp, op = ctypes.POINTER(native.GhostmCullHit), ctypes.POINTER(native.GhostmCullOut)
    for null in ("read_begin", "hit", "out"):
        rc = fn(len(rb) - 1, None if null == "read_begin" else rb.ctypes.data_as(u32p), len(h),
                None if null == "hit" else h.ctypes.data_as(hp), top_k, pct,
                None if null == "out" else out.ctypes.data_as(op))
        assert rc == 1 and "null: " in native.last_error(), (null, native.last_error())
    assert not out.view(np.uint32).any()
    assert fn(0, None, 0, None, 1, 50, None) == 0   # nothing to do needs no pointer
