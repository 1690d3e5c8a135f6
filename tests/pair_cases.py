"""Cases of the mate-pair join (PairJoinGpu, GhostmPairJoinHost; the contract is
above PairJoinGpu in include/ghostm_hip.h) and an independent model of it.

The model works on the whole mate-1 x mate-2 matrix of a pair at once: the
concordance of every (i, j), the row maxima and their first columns, the
column-wise smallest chooser. It shares nothing with pair_join.h, which runs
lane by lane over mate 2 as the kernel does.

A case is (pair_begin, offset, hits, max_span, orient): pair p's hits are
hits[pair_begin[2p]:pair_begin[2p + 1]] of mate 1 and
hits[pair_begin[2p + 1]:pair_begin[2p + 2]] of mate 2."""
import ctypes
import random

import numpy as np

from ghostm_amd import native
from ghostm_amd import LCA_HIT_DTYPE, PAIR_HIT_DTYPE, PAIR_OUT_DTYPE

NONE = 0xFFFFFFFF
TOP = (1 << 24) - 1   # the largest score, coordinate and offset
FILL = 0xC3C3C3C3      # what the refusal tests put into the outputs


def hits_of(rows):
    """rows of (subject, node, score, q_lo, q_hi, s_lo, s_hi, strand)"""
    h = np.zeros(len(rows), dtype=PAIR_HIT_DTYPE)
    for k, row in enumerate(rows):
        h[k] = tuple(row)
    return h


def one_pair(rows1, rows2, offset=100, max_span=500, orient=1):
    return (np.array([0, len(rows1), len(rows1) + len(rows2)], dtype=np.uint32), np.array([offset], dtype=np.uint32),
            hits_of(list(rows1) + list(rows2)), max_span, orient)


def join(cases, max_span, orient):
    """the pairs of several cases as one call's"""
    begin, parts, offs, at = [0], [], [], 0
    for pb, off, h, _, _ in cases:
        for p in range(len(off)):
            for half in (0, 1):
                lo, hi = int(pb[2 * p + half]), int(pb[2 * p + half + 1])
                parts.append(h[lo:hi])
                at += hi - lo
                begin.append(at)
            offs.append(int(off[p]))
    hits = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_HIT_DTYPE)
    return np.array(begin, dtype=np.uint32), np.array(offs, dtype=np.uint32), hits, max_span, orient


# ------------------------------------------------------------------ the model
def model(pair_begin, offset, hits, max_span, orient, info=None):
    """(cand, partner, pairs) as the calls return them. info, if a dict, gets
    counts over the call: joined, taken, ties (mate-1 candidates with two
    concordant partners of the best score) and discordant (candidate pairs on
    one subject that are not concordant)."""
    npairs = len(offset)
    cand = np.zeros(len(hits), dtype=LCA_HIT_DTYPE)
    partner = np.full(len(hits), NONE, dtype=np.uint32)
    pairs = np.zeros(npairs, dtype=PAIR_OUT_DTYPE)
    count = {"joined": 0, "taken": 0, "ties": 0, "discordant": 0}
    for p in range(npairs):
        b, m, e = (int(pair_begin[2 * p + k]) for k in range(3))
        off = int(offset[p])
        h1, h2 = hits[b:m], hits[m:e]
        f1 = {f: h1[f].astype(np.int64) for f in PAIR_HIT_DTYPE.names}
        f2 = {f: h2[f].astype(np.int64) for f in PAIR_HIT_DTYPE.names}
        c1, c2 = f1["score"] > 0, f2["score"] > 0
        both = c1[:, None] & c2[None, :]
        same = both & (f1["subject"][:, None] == f2["subject"][None, :])
        span = (np.maximum(f1["s_hi"][:, None], f2["s_hi"][None, :])
                - np.minimum(f1["s_lo"][:, None], f2["s_lo"][None, :]) + 1)
        conc = same & (span <= max_span)
        if orient:
            conc &= f1["strand"][:, None] != f2["strand"][None, :]
        count["discordant"] += int((same & ~conc).sum())
        best_key, best_span, joined = None, 0, 0
        score_out = 0
        chooser = {}
        if len(h1) and len(h2):
            S = np.where(conc, f2["score"][None, :], 0)
            top = S.max(axis=1)
            first = S.argmax(axis=1)   # the first column of the maximum
            count["ties"] += int(((S == top[:, None]).sum(axis=1)[top > 0] > 1).sum())
        else:
            top = np.zeros(len(h1), dtype=np.int64)
            first = np.zeros(len(h1), dtype=np.int64)
        for i in range(len(h1)):
            if not c1[i]:
                continue
            if top[i] > 0:
                j = int(first[i])
                total = int(f1["score"][i] + top[i])
                cand[b + i] = (h1["node"][i], total, h1["q_lo"][i], off + int(f2["q_hi"][j]))
                partner[b + i] = m + j
                chooser.setdefault(j, i)   # i ascends: the first is the lowest
                joined += 1
                key = (total, -i)
                if best_key is None or key > best_key:
                    best_key, best_span = key, int(span[i, j])
            else:
                cand[b + i] = (h1["node"][i], h1["score"][i], h1["q_lo"][i], h1["q_hi"][i])
            score_out = max(score_out, int(cand["score"][b + i]))
        for j in range(len(h2)):
            if not c2[j]:
                continue
            if j in chooser:
                partner[m + j] = b + chooser[j]
            else:
                cand[m + j] = (h2["node"][j], h2["score"][j], int(f2["q_lo"][j]) + off, int(f2["q_hi"][j]) + off)
                score_out = max(score_out, int(f2["score"][j]))
        pairs[p] = (joined, int(c1.any()) | (int(c2.any()) << 1), score_out, best_span)
        count["joined"] += joined
        count["taken"] += len(chooser)
    if info is not None:
        info.update(count)
    return cand, partner, pairs


# --------------------------------------------------------------------- shapes
A, B, C = 7, 8, 9             # subjects
NA, NB, NC = 70, 80, NONE     # their nodes (C has none)


def hit(subject, score, s_lo, s_hi, strand, q_lo=0, q_hi=49):
    node = {A: NA, B: NB, C: NC}[subject]
    return (subject, node, score, q_lo, q_hi, s_lo, s_hi, strand)


def shape_cases():
    """name -> case; expected_shapes() knows what each must give"""
    s = {}
    s["empty_pair"] = one_pair([], [])
    s["only_mate1"] = one_pair([hit(A, 50, 100, 149, 0), hit(B, 40, 10, 59, 1)], [])
    s["only_mate2"] = one_pair([], [hit(A, 50, 100, 149, 1, 5, 44)])
    s["joined"] = one_pair([hit(A, 100, 100, 149, 0, 3, 47)], [hit(A, 80, 300, 349, 1, 2, 40)])
    s["two_choose_one"] = one_pair([hit(A, 60, 100, 149, 0), hit(A, 90, 120, 169, 0)], [hit(A, 80, 300, 349, 1)])
    s["score_tie"] = one_pair([hit(A, 60, 100, 149, 0)],
                              [hit(A, 70, 500, 549, 1), hit(A, 80, 300, 349, 1), hit(A, 80, 200, 249, 1)])
    s["span_at_max"] = one_pair([hit(A, 60, 100, 149, 0)], [hit(A, 80, 550, 599, 1)], max_span=500)
    s["span_over_max"] = one_pair([hit(A, 60, 100, 149, 0)], [hit(A, 80, 551, 600, 1)], max_span=500)
    s["mate2_left_of_mate1"] = one_pair([hit(A, 60, 551, 600, 1)], [hit(A, 80, 101, 150, 0)], max_span=500)
    s["same_strand_orient1"] = one_pair([hit(A, 60, 100, 149, 1)], [hit(A, 80, 300, 349, 1)], orient=1)
    s["same_strand_orient0"] = one_pair([hit(A, 60, 100, 149, 1)], [hit(A, 80, 300, 349, 1)], orient=0)
    s["non_candidate_between"] = one_pair(
        [hit(A, 60, 100, 149, 0), hit(A, 0, 100, 149, 0), hit(B, 40, 10, 59, 0)],
        [hit(B, 0, 100, 149, 1), hit(A, 0, 300, 349, 1), hit(A, 30, 320, 369, 1)])
    s["same_subject_not_concordant"] = one_pair([hit(A, 60, 100, 149, 0), hit(B, 50, 10, 59, 0)],
                                                [hit(A, 80, 5000, 5049, 1), hit(B, 45, 20, 69, 0)])
    s["no_node"] = one_pair([hit(C, 60, 100, 149, 0)], [hit(C, 80, 300, 349, 1)])
    s["largest_values"] = one_pair([(A, NA, TOP, 0, TOP, 0, TOP, 0)], [(A, NA, TOP, TOP, TOP, 0, TOP, 1)], offset=TOP,
                                   max_span=1 << 24)
    return s


def expected_shapes(name, got):
    """what the contract says of the shapes, word by word where it is short"""
    cand, partner, pairs = got
    c, p, o = [tuple(int(v) for v in r) for r in cand], [int(v) for v in partner], [tuple(int(v) for v in r) for r in pairs]
    if name == "empty_pair":
        assert o == [(0, 0, 0, 0)] and not c
    elif name == "only_mate1":
        assert c == [(NA, 50, 0, 49), (NB, 40, 0, 49)] and p == [NONE, NONE] and o == [(0, 1, 50, 0)]
    elif name == "only_mate2":
        assert c == [(NA, 50, 105, 144)] and p == [NONE] and o == [(0, 2, 50, 0)]
    elif name == "joined":
        assert c == [(NA, 180, 3, 140), (0, 0, 0, 0)] and p == [1, 0] and o == [(1, 3, 180, 250)]
    elif name == "two_choose_one":   # the taken hit names the lower chooser; best_span is the higher score's
        assert c == [(NA, 140, 0, 149), (NA, 170, 0, 149), (0, 0, 0, 0)] and p == [2, 2, 0]
        assert o == [(2, 3, 170, 230)]
    elif name == "score_tie":   # the lower index of the two 80s; the others stay candidates of their own
        assert p == [2, NONE, 0, NONE] and c[0] == (NA, 140, 0, 149) and c[2] == (0, 0, 0, 0)
        assert c[1] == (NA, 70, 100, 149) and c[3] == (NA, 80, 100, 149) and o == [(1, 3, 140, 250)]
    elif name in ("span_at_max", "mate2_left_of_mate1"):
        assert o == [(1, 3, 140, 500)] and p == [1, 0]
    elif name in ("span_over_max", "same_strand_orient1"):
        assert o == [(0, 3, 80, 0)] and p == [NONE, NONE] and c == [(NA, 60, 0, 49), (NA, 80, 100, 149)]
    elif name == "same_strand_orient0":
        assert o == [(1, 3, 140, 250)] and p == [1, 0]
    elif name == "non_candidate_between":
        assert p == [5, NONE, NONE, NONE, NONE, 0] and o == [(1, 3, 90, 270)]
        assert c == [(NA, 90, 0, 149), (0, 0, 0, 0), (NB, 40, 0, 49), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    elif name == "same_subject_not_concordant":   # A too far, B on one strand
        assert o == [(0, 3, 80, 0)] and p == [NONE] * 4
    elif name == "no_node":
        assert c[0] == (NONE, 140, 0, 149) and o == [(1, 3, 140, 250)]
    elif name == "largest_values":
        assert c[0] == (NA, 2 * TOP, 0, 2 * TOP) and o == [(1, 3, 2 * TOP, 1 << 24)]
    else:
        raise AssertionError("no expectation for " + name)


# ------------------------------------------------------------- random records
def random_rows(rnd, n, subjects=5, zero_rate=0.15):
    """n hits on a few subjects, scores from a small range (ties), subject
    ranges spread so that about half the same-subject pairs are within 600"""
    rows = []
    for _ in range(n):
        sub = rnd.randrange(subjects)
        score = 0 if rnd.random() < zero_rate else rnd.choice((20, 30, 30, 40, rnd.randrange(1, 200)))
        s_lo = rnd.randrange(0, 1200)
        q_lo = rnd.randrange(0, 60)
        rows.append((sub, NONE if sub == 0 else 10 + sub, score, q_lo, q_lo + rnd.randrange(0, 90), s_lo,
                     s_lo + rnd.randrange(0, 150), rnd.randrange(2)))
    return rows


SIZES = (64, 65, 1024, 1025, 3000)   # the class borders, in hits, and one in the device-memory class


def sized_pair(n, seed=0):
    """One pair of n hits, mate 1 a little shorter than mate 2, subjects in
    proportion so that a mate-1 hit has a handful of concordant partners."""
    rnd = random.Random(20270101 + 7 * n + seed)
    n1 = n // 2 - n // 9
    subjects = max(2, n // 12)
    return one_pair(random_rows(rnd, n1, subjects), random_rows(rnd, n - n1, subjects), offset=150, max_span=600,
                    orient=n % 2)


def mixed_call(max_span=600, orient=1):
    """every class in one call, pairs without hits and with one mate between them"""
    empty = one_pair([], [])
    rnd = random.Random(20270102)
    left = one_pair(random_rows(rnd, 70, 4), [])
    right = one_pair([], random_rows(rnd, 9, 4))
    parts = [sized_pair(5, 1), sized_pair(1025, 1), sized_pair(64, 1), empty, sized_pair(300, 1), sized_pair(65, 1), left,
             sized_pair(2, 1), sized_pair(1100, 1), empty, right, sized_pair(700, 1), sized_pair(63, 1)]
    return join(parts, max_span, orient)


def random_calls(count, seed=20270103):
    """count calls of a few pairs each"""
    rnd = random.Random(seed)
    calls = []
    for _ in range(count):
        pairs = []
        for _ in range(rnd.randrange(1, 6)):
            n1, n2 = rnd.choice((0, 1, 2, 3, 8, 20, 40)), rnd.choice((0, 1, 2, 3, 8, 20, 45))
            pairs.append(one_pair(random_rows(rnd, n1), random_rows(rnd, n2), offset=rnd.choice((0, 1, 100, 151))))
        calls.append(join(pairs, rnd.choice((1, 150, 600, 600, 1 << 24)), rnd.randrange(2)))
    return calls


def assert_same(got, want, what):
    for g, w, part in zip(got, want, ("cand", "partner", "pairs")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {len(bad)} {part} entries differ, first {bad[0]}: {g[bad[0]]} != {w[bad[0]]}")


# ------------------------------------------------------------------- refusals
def refusals():
    """(reason, pair_begin, offset, hits, max_span, orient): every reason of the contract but "null" """
    h = hits_of([hit(A, 50, 100, 149, 0), hit(B, 40, 10, 59, 1), hit(A, 30, 300, 349, 1), hit(B, 20, 30, 90, 0)])

    def changed(k, field, value):
        g = h.copy()
        g[field][k] = value
        return g

    pb = np.array([0, 2, 3, 3, 4], dtype=np.uint32)
    off = np.array([100, 120], dtype=np.uint32)
    many = np.zeros(16385, dtype=PAIR_HIT_DTYPE)
    return [
        ("reads", np.array([0, 3, 2, 3, 4], dtype=np.uint32), off, h, 500, 1),
        ("reads", np.array([0, 2, 3, 4, 3], dtype=np.uint32), off, h, 500, 1),
        ("reads", np.array([0, 2, 3, 3, 5], dtype=np.uint32), off, h, 500, 1),
        ("reads", np.array([0, 9000, 16385], dtype=np.uint32), off[:1], many, 500, 1),
        ("range", pb, off, changed(1, "q_lo", 50), 500, 1),
        ("range", pb, off, changed(2, "s_lo", 350), 500, 1),
        ("bounds", pb, off, changed(3, "q_hi", TOP + 1), 500, 1),
        ("bounds", pb, off, changed(0, "s_hi", TOP + 1), 500, 1),
        ("bounds", pb, off, changed(0, "score", TOP + 1), 500, 1),
        ("bounds", pb, off, changed(2, "strand", 2), 500, 1),
        ("bounds", pb, np.array([100, TOP + 1], dtype=np.uint32), h, 500, 1),
        ("param", pb, off, h, 0, 1),
        ("param", pb, off, h, (1 << 24) + 1, 1),
        ("param", pb, off, h, 500, 2),
    ]


def raw_call(fn, pb, off, h, max_span, orient, cand, partner, pairs, npairs=None, nhits=None):
    """the entry point itself; None for a null pointer"""
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    if npairs is None:
        npairs = 0 if pb is None else (len(pb) - 1) // 2
    if nhits is None:
        nhits = 0 if h is None else len(h)
    return fn(npairs, ptr(pb, u32p), ptr(off, u32p), nhits,
              ptr(h, ctypes.POINTER(native.GhostmPairHit)), max_span, orient,
              ptr(cand, ctypes.POINTER(native.GhostmLcaHit)), ptr(partner, u32p),
              ptr(pairs, ctypes.POINTER(native.GhostmPairOut)))


def filled_outputs(nhits, npairs):
    return (np.full(4 * nhits, FILL, dtype=np.uint32).view(LCA_HIT_DTYPE), np.full(nhits, FILL, dtype=np.uint32),
            np.full(4 * npairs, FILL, dtype=np.uint32).view(PAIR_OUT_DTYPE))


def check_refusals(fn_name):
    """Every reason on one entry point; the outputs keep their bytes."""
    fn = getattr(native.load(), fn_name)
    for reason, pb, off, h, max_span, orient in refusals():
        outs = filled_outputs(len(h), len(off))
        assert raw_call(fn, pb, off, h, max_span, orient, *outs) == 1, reason
        msg = native.last_error()
        assert msg.startswith(fn_name + ": ") and (reason + ": ") in msg, (reason, msg)
        for o in outs:
            assert (o.view(np.uint32) == FILL).all(), reason
    pb, off, h, max_span, orient = shape_cases()["joined"]
    for null in ("pair_begin", "offset", "hit", "cand", "partner", "out"):
        outs = list(filled_outputs(len(h), len(off)))
        args = [pb, off, h, max_span, orient] + outs
        args[{"pair_begin": 0, "offset": 1, "hit": 2, "cand": 5, "partner": 6, "out": 7}[null]] = None
        assert raw_call(fn, *args, npairs=1, nhits=len(h)) == 1 and "null: " in native.last_error(), (null, native.last_error())
        for o in outs:
            assert (o.view(np.uint32) == FILL).all(), null
    assert raw_call(fn, None, None, None, 500, 1, None, None, None) == 0   # nothing to do needs no pointer
