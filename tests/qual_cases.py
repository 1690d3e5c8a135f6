"""The quality stage's Python model and case sets (GhostmQualityTrimHost,
QualityTrimGpu; the rule is above GhostmQualityTrimHost in include/ghostm_hip.h).

The model is the issue's: each end by the running sum on the untrimmed read,
the floor, then the mask. The sets: the fixed lengths around the 64-position
groups of the kernel, about 300 random reads per parameter set with a high
plateau, a decaying 3' tail, a few low 5' letters and random dips, all laid at
odd byte offsets in one buffer with gap bytes between them (a gap's quality
byte is 0xFF and its letter '#': a kernel that read or wrote a byte beside its
read would count a bad byte or lose a '#'), and the carry cases by name.

check_sets() asserts that the sets hold what they are meant to. The classes a
random set must hold (20 reads each) depend on what its parameters can do:
with 0 < trim_q < 93, reads trimmed at both ends, untouched reads and reads
emptied by crossing ends; with min_len > 0, reads the floor empties although
the ends left them letters; with trim_q 0 nothing can be trimmed, so the set
must hold masked and unmasked reads instead; with trim_q 93 no sum ever falls
below 0, so a read is either all '~' (untouched) or emptied, and both are
there."""
import random

import numpy as np

PARAM_SETS = [(20, 0, 0), (2, 0, 0), (20, 10, 30), (0, 15, 0), (93, 0, 0)]
FIXED_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 1000]
OUT_DTYPE = np.dtype([("begin", "<u4"), ("kept", "<u4"), ("masked", "<u4"), ("bad", "<u4")])
GAP_LETTER, GAP_QUAL = ord("#"), 0xFF


# ------------------------------------------------------------------ the model
def trim(q, t):  # q: list of Phred ints
    def walk(idx):
        s = best = 0
        at = None
        for i in idx:
            s += t - q[i]
            if s < 0:
                break
            if s > best:
                best, at = s, i
        return at
    e = walk(range(len(q) - 1, -1, -1))
    b = walk(range(len(q)))
    end = len(q) if e is None else e
    begin = 0 if b is None else b + 1
    return (begin, end - begin) if end > begin else (0, 0)


def phred(qual: bytes):
    return [min(max(b, 33), 126) - 33 for b in qual]


def model_read(letters: bytes, qual: bytes, params):
    """(letters after the stage, (begin, kept, masked, bad), (trimmed5, trimmed3, failed))"""
    t, m, floor = params
    n = len(letters)
    bad = sum(1 for b in qual if b < 33 or b > 126)
    if not (t or m or floor):  # off: the qualities are not read
        return letters, (0, n, 0, 0), (0, 0, 0)
    q = phred(qual)
    begin, kept = trim(q, t)
    failed = kept < floor
    if failed:
        begin = kept = 0
    out = bytearray(letters)
    masked = 0
    for i in range(begin, begin + kept):
        if q[i] < m:
            out[i] = ord("N")
            masked += 1
    sums = (begin if kept else 0, n - begin - kept if kept else n, int(failed))
    return bytes(out), (begin, kept, masked, bad), sums


def model(letters: bytes, qual: bytes, offs, lens, params):
    """The stage on a laid-out buffer: (letters, OUT_DTYPE records, the counters' sums)."""
    buf = bytearray(letters)
    out = np.zeros(len(offs), dtype=OUT_DTYPE)
    sums = dict(trimmed5=0, trimmed3=0, masked=0, failed=0, bad=0, reads=len(offs), letters=int(sum(lens)))
    on = any(params)
    for r, (o, n) in enumerate(zip(offs, lens)):
        o, n = int(o), int(n)
        new, rec, (t5, t3, failed) = model_read(bytes(buf[o:o + n]), qual[o:o + n], params)
        buf[o:o + n] = new
        out[r] = rec
        if on:
            sums["trimmed5"] += t5
            sums["trimmed3"] += t3
            sums["masked"] += rec[2]
            sums["failed"] += failed
            sums["bad"] += rec[3]
    return bytes(buf), out, sums


# ------------------------------------------------------------------ laying out
def lay_out(reads, seed=1):
    """reads: (letters, quality bytes) pairs -> (letters, qual, offsets, lengths), every read at an odd offset
    behind 1..4 gap bytes, and gap bytes at the end."""
    rnd = random.Random(seed)
    letters, qual, offs, lens = bytearray(), bytearray(), [], []
    for ls, qs in reads:
        assert len(ls) == len(qs)
        gap = rnd.randint(1, 4)
        if (len(letters) + gap) % 2 == 0:
            gap += 1
        letters += bytes([GAP_LETTER]) * gap
        qual += bytes([GAP_QUAL]) * gap
        offs.append(len(letters))
        lens.append(len(ls))
        letters += ls
        qual += qs
    letters += bytes([GAP_LETTER]) * 3
    qual += bytes([GAP_QUAL]) * 3
    return bytes(letters), bytes(qual), np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def gaps_untouched(letters: bytes, offs, lens) -> bool:
    inside = np.zeros(len(letters), dtype=bool)
    for o, n in zip(offs, lens):
        inside[int(o):int(o) + int(n)] = True
    return bool((np.frombuffer(letters, dtype=np.uint8)[~inside] == GAP_LETTER).all())


def rand_letters(rnd, n):
    return bytes(rnd.choice(b"ACGTACGTACGTN") for _ in range(n))


def to_qual(q):
    return bytes(v + 33 for v in q)


# ------------------------------------------------------------------ random sets
def profile(rnd, n, kind, t):
    """n Phred scores: a plateau above t (or at 93 when t is 93) with the kind's ends."""
    hi = lambda: 93 if t >= 93 else rnd.randint(t + 5, min(93, t + 20))  # noqa: E731
    lo = lambda: rnd.randint(0, t - 1)  # noqa: E731
    q = [hi() for _ in range(n)]
    if kind == "untouched":
        # half of them with dips well inside: each walk stops at the read's first good end letter
        for _ in range(n // 40 if rnd.random() < 0.5 else 0):
            p = rnd.randint(10, n - 11) if n > 30 else None
            if p is not None:
                q[p] = lo()
    elif kind in ("both", "tail", "short"):
        core = rnd.randint(5, 25) if kind == "short" else max(n - rnd.randint(5, 40), n // 2)
        core = min(core, n)
        head = rnd.randint(1, 4) if kind != "tail" and n - core >= 2 else 0
        head = min(head, n - core)
        tail = n - core - head
        for i in range(head):
            q[i] = lo()
        for k in range(tail):  # decaying: the further out, the lower
            i = n - 1 - k
            q[i] = lo() if k < tail - 3 or t >= 93 else min(t - 1, rnd.randint(max(t - 6, 0), t - 1))
    elif kind == "crossing":
        q = [lo() for _ in range(n)]
    return q


def random_set(params, seed=0):
    """(reads, kinds): the fixed lengths, then about 300 random reads, for this parameter set."""
    t = params[0] or 20
    rnd = random.Random(1000 * seed + 7 * params[0] + 3 * params[1] + params[2])
    kinds = ["untouched", "both", "tail", "crossing", "short"]
    reads, kind_of = [], []
    for n in FIXED_LENGTHS:
        for kind in ("untouched", "both", "crossing"):
            q = profile(rnd, n, kind, t) if n else []
            reads.append((rand_letters(rnd, n), to_qual(q)))
            kind_of.append(kind)
    for k in range(300):
        kind = kinds[k % len(kinds)]
        n = rnd.randint(40, 300)
        reads.append((rand_letters(rnd, n), to_qual(profile(rnd, n, kind, t))))
        kind_of.append(kind)
    return reads, kind_of


def classes(reads, params):
    """How many reads of each class the model finds."""
    t, m, floor = params
    c = dict(both=0, untouched=0, crossing=0, floor=0, masked=0, unmasked=0)
    for ls, qs in reads:
        n = len(ls)
        if n == 0:
            continue
        begin, kept = trim(phred(qs), t)
        _, rec, _ = model_read(ls, qs, params)
        c["both"] += begin > 0 and 0 < kept < n - begin
        c["untouched"] += begin == 0 and kept == n
        c["crossing"] += kept == 0
        c["floor"] += 0 < kept < floor
        c["masked"] += rec[2] > 0
        c["unmasked"] += rec[1] > 0 and rec[2] == 0
    return c


# ------------------------------------------------------------------ the carry cases
def oriented(walk_q, end3: bool, n: int, fill: int = 40):
    """A read of n scores whose walk from the 3' end (end3) or the 5' end meets walk_q in order; the rest is fill."""
    assert len(walk_q) <= n
    q = list(walk_q) + [fill] * (n - len(walk_q))
    return q[::-1] if end3 else q


def cut_at(q, end3: bool, t: int):
    """The walked index (0 = the end's first letter) the model cuts at, or None."""
    begin, kept = trim(q, t)
    n = len(q)
    if end3:
        return None if begin + kept == n else n - 1 - (begin + kept)
    return None if begin == 0 else begin - 1


def carry_cases():
    """name -> (reads, params, check(out records)); trim_q 20: q 19 adds 1, 21 takes 1, 20 adds 0, 0 adds 20, 40 takes 20."""
    up, down, flat = 19, 21, 20
    rnd = random.Random(99)
    cases = {}

    def walk_case(name, walk_q, want_k, n=200):
        for end3 in (True, False):
            q = oriented(walk_q, end3, n)
            assert cut_at(q, end3, 20) == want_k, name
            assert cut_at(q, not end3, 20) is None  # the other end is good: that walk stops at once

            def check(out, end3=end3, want_k=want_k, n=n):
                if end3:
                    assert (int(out[0]["begin"]), int(out[0]["kept"])) == (0, n - 1 - want_k)
                else:
                    assert (int(out[0]["begin"]), int(out[0]["kept"])) == (want_k + 1, n - want_k - 1)
            cases[f"{name}_{'3p' if end3 else '5p'}"] = ([(rand_letters(rnd, n), to_qual(q))], (20, 0, 0), check)

    # the best sum at lane 63 of the first group, and at lane 0 of the next
    walk_case("best_at_lane63", [up] * 64 + [down] * 70, 63)
    walk_case("best_at_lane0_of_next_group", [up] * 65 + [down] * 70, 64)
    # an equal best in two groups: 10 at walked 9 and again at walked 79; the first walked wins
    walk_case("equal_best_in_two_groups", [up] * 10 + [down] * 10 + [flat] * 50 + [up] * 10 + [down] * 12, 9)
    # the stop at lane 0 of the second group, far larger sums behind it
    walk_case("stop_at_lane0_hides_larger", [up] * 10 + [down] * 10 + [flat] * 44 + [down] + [0] * 60, 9)
    # the sum returns to exactly 0 (no stop) and rises higher afterwards
    walk_case("sum_returns_to_zero", [up] * 5 + [down] * 5 + [up] * 8 + [40], 17)
    # a best in the third group, reached over a long flat stretch
    walk_case("best_in_third_group", [up] * 3 + [flat] * 140 + [up] * 2 + [down] * 6, 144)

    def simple(name, reads, params, check):
        cases[name] = (reads, params, check)

    def expect(fields, want):
        def check(out):
            got = [[int(x) for x in out[f]] for f in fields]
            assert got == want, (got, want)
        return check

    n = 150
    assert trim([2] * n, 20) == (0, 0) and cut_at([2] * n, True, 20) == n - 1  # end == 0
    simple("all_bad", [(rand_letters(rnd, n), to_qual([2] * n))], (20, 0, 0), expect(("begin", "kept"), [[0], [0]]))
    simple("all_good", [(rand_letters(rnd, n), to_qual([40] * n))], (20, 0, 0), expect(("begin", "kept"), [[0], [n]]))
    q = [rnd.randint(0, 40) for _ in range(n)]
    simple("trim_off_mask_on", [(rand_letters(rnd, n), to_qual(q))], (0, 15, 0),
           expect(("begin", "kept", "masked"), [[0], [n], [sum(v < 15 for v in q)]]))
    q = oriented([3] * 30, True, n)  # everything kept becomes N; the trimmed tail is not rewritten
    simple("mask_above_every_score", [(rand_letters(rnd, n), to_qual(q))], (20, 93, 0),
           expect(("begin", "kept", "masked"), [[0], [n - 30], [n - 30]]))
    qual = bytearray(to_qual([40] * n))
    qual[70], qual[71], qual[0] = 32, 127, 127  # 32 scores 0 and 127 scores 93; each counts as bad
    simple("bad_bytes", [(rand_letters(rnd, n), bytes(qual))], (20, 10, 0), expect(("bad", "masked"), [[3], [1]]))
    empties = [(b"", b""), (rand_letters(rnd, 70), to_qual([40] * 60 + [2] * 10)), (b"", b""), (b"", b"")]
    simple("empty_reads", empties, (20, 0, 0), expect(("kept",), [[0, 60, 0, 0]]))
    simple("empty_reads_with_a_floor", empties, (20, 0, 61), expect(("kept",), [[0, 0, 0, 0]]))
    return cases


def grid_stride_set(n_reads=4500):
    """More reads than a launch has waves (4 x 1024): short reads of every small length."""
    rnd = random.Random(5)
    reads = []
    for k in range(n_reads):
        n = k % 23
        q = [rnd.choice((2, 19, 21, 40)) for _ in range(n)]
        reads.append((rand_letters(rnd, n), to_qual(q)))
    return reads


# ------------------------------------------------------------------ what the sets must hold
def check_sets():
    for params in PARAM_SETS:
        reads, _ = random_set(params)
        lengths = [len(x[0]) for x in reads]
        assert all(n in lengths for n in FIXED_LENGTHS) and 300 <= len(reads) <= 340
        letters, qual, offs, lens = lay_out(reads)
        assert all(int(o) % 2 == 1 for o in offs) and gaps_untouched(letters, offs, lens)
        assert all(33 <= b <= 126 for _, qs in reads for b in qs)
        c = classes(reads, params)
        t, m, floor = params
        if 0 < t < 93:
            assert min(c["both"], c["untouched"], c["crossing"]) >= 20, (params, c)
        elif t == 0:
            assert c["both"] == 0 and c["crossing"] == 0 and min(c["masked"], c["unmasked"]) >= 20, (params, c)
        else:
            assert min(c["untouched"], c["crossing"]) >= 20, (params, c)
        if floor:
            assert c["floor"] >= 20, (params, c)
        if m and t:
            assert c["masked"] >= 20, (params, c)
        new, out, sums = model(letters, qual, offs, lens, params)
        assert gaps_untouched(new, offs, lens) and sums["bad"] == 0
    cc = carry_cases()
    assert len(cc) == 12 + 7
    for name, (reads, params, check) in cc.items():
        letters, qual, offs, lens = lay_out(reads)
        _, out, _ = model(letters, qual, offs, lens, params)
        check(out)
    assert len(grid_stride_set()) > 4 * 1024
