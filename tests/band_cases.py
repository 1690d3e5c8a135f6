"""Shared by tests/test_band_align_host.py, tests/test_gpu_band_align.py and
tests/band_poison_child.py (not a test module): a Python model of the
read-level banded alignment written from its contract, the checker that
re-walks a path along the two sequences, an unbanded Smith-Waterman-Gotoh
score for tiny inputs, the builder of tile records and the stage cases.

The contract (include/ghostm_hip.h, BandAlignGpu). Per hit: a source of m
letters q[0..m), a subject range [s_lo, s_hi] absolute in the DB chunk, an
anchor diagonal D and a half-width B. The band cells are (i, j) with 0 <= i <
m, s_lo <= j <= s_hi, |j - i - D| <= B. Reverse DP, rows i = m-1..0, j
descending in a row, all int32:
    s      = H(i+1,j+1) + M[db[j]*32 + q[i]]
    E(i,j) = max(E(i,j+1) + ext, H(i,j+1) + open)     'D'
    F(i,j) = max(F(i+1,j) + ext, H(i+1,j) + open)     'I'
    H(i,j) = s if s > 0 else 0; then E if E > H; then F if F > H (hsel 0/1/2/3)
    eext   = E(i,j+1) + ext > H(i,j+1) + open (a tie opens); fext likewise
A neighbour that is no band cell has H = 0 and E = F = minus infinity. The
start cell is the first strict maximum in processing order; the walk:
    H, hsel 1   emit '=' / 'X', go to H(i+1, j+1)
    H, hsel 2/3 enter E / F at the same cell
    H, hsel 0   stop; leaving the band cells stops
    E           emit 'D', go to E(i, j+1) if eext else H(i, j+1)
    F           emit 'I', go to F(i+1, j) if fext else H(i+1, j)
Score 0: an empty path at q_start = 0, s_start = s_lo."""
from __future__ import annotations

import ctypes
import itertools
import random
import re

import numpy as np

import tile_cases as tc

AA = "ARNDCQEGHILKMFPSTWYV"
END = 25
OPS = "=XID"
NEG = -(1 << 29)


# ---------------------------------------------------------------- small helpers
def codes(s: str) -> np.ndarray:
    return np.array([AA.index(c) for c in s], dtype=np.uint8)


def rand_seq(rnd, n: int) -> str:
    return "".join(rnd.choice(AA) for _ in range(n))


def mutate(rnd, s: str, rate: float) -> str:
    return "".join(rnd.choice(AA) if rnd.random() < rate else c for c in s)


def runs(ops: str) -> list:
    """The run-length words (length << 4 | op) of an operation string."""
    return [len(list(g)) << 4 | OPS.index(c) for c, g in itertools.groupby(ops)]


def expand(words) -> str:
    return "".join(OPS[int(w) & 3] * (int(w) >> 4) for w in words)


def hit_words(rec, ops, h):
    o = int(rec["ops_offset"][h])
    return ops[o:o + int(rec["n_runs"][h])]


# ---------------------------------------------------------------- Python model
def band_model(sources, db, M, D, s_lo, s_hi, B, open_gap=-11, extend_gap=-1):
    """All hits of a case at once (numpy over the hits; the rows and the E chain
    of a row run one after the other, as the recurrence says). sources: one
    code array per hit. Returns a list of dict(score, q_start, q_end, s_start,
    s_end, ops) with ops the operation string."""
    n, lanes = len(sources), 2 * B + 1
    m = np.array([len(q) for q in sources], dtype=np.int64)
    mmax = int(m.max())
    Q = np.zeros((n, mmax), dtype=np.int64)
    for h, q in enumerate(sources):
        Q[h, :len(q)] = np.asarray(q, dtype=np.int64) & 31
    db = np.asarray(db, dtype=np.int64)
    M2 = np.asarray(M, dtype=np.int64).reshape(32, 32)
    D = np.asarray(D, dtype=np.int64)
    lo = np.asarray(s_lo, dtype=np.int64)
    hi = np.asarray(s_hi, dtype=np.int64)
    lane = np.arange(lanes, dtype=np.int64)
    Hp = np.zeros((n, lanes), dtype=np.int64)
    Fp = np.full((n, lanes), NEG, dtype=np.int64)
    dirs = np.zeros((mmax, n, lanes), dtype=np.uint8)
    best = np.zeros(n, dtype=np.int64)
    bi = np.zeros(n, dtype=np.int64)
    bj = lo.copy()
    zero = np.zeros((n, 1), dtype=np.int64)
    neg = np.full((n, 1), NEG, dtype=np.int64)
    for i in range(mmax - 1, -1, -1):
        j = i + D[:, None] - B + lane[None, :]
        cell_ok = (i < m)[:, None] & (j >= lo[:, None]) & (j <= hi[:, None])
        sub = M2[db[np.clip(j, 0, len(db) - 1)] & 31, Q[:, i][:, None]]
        s = Hp + sub                                         # H(i+1, j+1): the same lane, one row back
        Hb = np.concatenate([zero, Hp[:, :-1]], axis=1)      # (i+1, j): lane b - 1, one row back
        Fb = np.concatenate([neg, Fp[:, :-1]], axis=1)
        fe, fo = Fb + extend_gap, Hb + open_gap
        F = np.maximum(fe, fo)
        Hc = np.zeros((n, lanes + 1), dtype=np.int64)        # column `lanes`: past the band, no cell
        Ec = np.full((n, lanes + 1), NEG, dtype=np.int64)
        for b in range(lanes - 1, -1, -1):
            ee, eo = Ec[:, b + 1] + extend_gap, Hc[:, b + 1] + open_gap
            E = np.maximum(ee, eo)
            sb = s[:, b]
            cell = np.where(sb > 0, sb, 0)
            sel = (sb > 0).astype(np.int64)
            t = E > cell
            cell, sel = np.where(t, E, cell), np.where(t, 2, sel)
            t = F[:, b] > cell
            cell, sel = np.where(t, F[:, b], cell), np.where(t, 3, sel)
            ok = cell_ok[:, b]
            Hc[:, b] = np.where(ok, cell, 0)
            Ec[:, b] = np.where(ok, E, NEG)
            dirs[i, :, b] = np.where(ok, sel | (ee > eo) << 2 | (fe[:, b] > fo[:, b]) << 3, 0)
        Hrow = Hc[:, :lanes]
        rowmax = Hrow.max(axis=1)
        # j descends in a row: the first cell of the row's maximum is its largest lane
        arg = lanes - 1 - np.argmax(Hrow[:, ::-1] == rowmax[:, None], axis=1)
        upd = rowmax > best
        best = np.where(upd, rowmax, best)
        bi = np.where(upd, i, bi)
        bj = np.where(upd, i + D - B + arg, bj)
        Hp = Hrow
        Fp = np.where(cell_ok, F, NEG)

    out = []
    for h in range(n):
        q = Q[h]
        i, j, state, ops = int(bi[h]), int(bj[h]), "H", []

        def at(i, j):
            b = j - i - int(D[h]) + B
            if i >= m[h] or j > hi[h] or j < lo[h] or b < 0 or b >= lanes:
                return None
            return int(dirs[i, h, b])

        if best[h] > 0:
            while True:
                d = at(i, j)
                if d is None:
                    break
                if state == "H":
                    if d & 3 == 0:
                        break
                    if d & 3 == 1:
                        ops.append("=" if int(db[j]) == int(sources[h][i]) else "X")
                        i, j = i + 1, j + 1
                    else:
                        state = "E" if d & 3 == 2 else "F"
                elif state == "E":
                    ops.append("D")
                    state = "E" if d & 4 else "H"
                    j += 1
                else:
                    ops.append("I")
                    state = "F" if d & 8 else "H"
                    i += 1
        out.append(dict(score=int(best[h]), q_start=int(bi[h]), s_start=int(bj[h]),
                        q_end=i - 1 if best[h] > 0 else int(bi[h]), s_end=j - 1 if best[h] > 0 else int(bj[h]),
                        ops="".join(ops)))
    return out


def assert_equals_model(rec, ops, model):
    """(rec, ops) of a host or device call against band_model's list."""
    assert len(rec) == len(model)
    for h, r in enumerate(model):
        got = tuple(int(rec[f][h]) for f in ("q_start", "q_end", "s_start", "s_end", "score"))
        assert got == (r["q_start"], r["q_end"], r["s_start"], r["s_end"], r["score"]), (h, got, r)
        assert list(hit_words(rec, ops, h)) == runs(r["ops"]), (h, r["ops"])
    n_runs = np.asarray(rec["n_runs"], dtype=np.int64)
    assert np.array_equal(rec["ops_offset"], np.concatenate([[0], np.cumsum(n_runs)[:-1]]).astype(np.uint64))
    assert len(ops) == int(n_runs.sum())


# ---------------------------------------------------------------- the checker
def adjacent_gaps_excluded(M, open_gap) -> bool:
    """A 'D' run next to an 'I' run costs at least 2 * open; one pair column in
    their place costs the pair's matrix entry. Where every entry among the
    residue codes is above 2 * open the recurrence never puts the two kinds of
    run side by side (BLOSUM62 11/1, PAM250 14/2); with cheap gaps (open ==
    extend == -1 against a -4 mismatch) it may."""
    M2 = np.asarray(M, dtype=np.int64).reshape(32, 32)
    return int(M2[:20, :20].min()) > 2 * open_gap


def check_band_path(q, db, M, r, words, D, B, s_lo, s_hi, open_gap, extend_gap):
    """Re-walks one hit's path along the two sequences: rescore equals score,
    every cell lies inside the band cells, the first and last operations are
    pair columns, no 'I' run is adjacent to a 'D' run (where the scoring
    excludes it), q_end, s_end and n_runs are consistent. r: the hit's record
    (absolute subject coordinates). Returns the operation string."""
    M = M if isinstance(M, list) else [int(x) for x in np.asarray(M).reshape(-1)]
    m = len(q)
    assert int(r["n_runs"]) == len(words)
    if int(r["score"]) == 0:
        assert len(words) == 0 and int(r["q_end"]) == int(r["q_start"]) == 0
        assert int(r["s_end"]) == int(r["s_start"]) == s_lo
        return ""
    for a, b in zip(words[:-1], words[1:]):
        assert (int(a) & 15) != (int(b) & 15)  # maximal runs
    assert all(int(w) & 12 == 0 and int(w) >> 4 > 0 for w in words)
    ops = expand(words)
    i, j, score, prev = int(r["q_start"]), int(r["s_start"]), 0, None

    def inside(i, j):
        return 0 <= i < m and s_lo <= j <= s_hi and abs(j - i - D) <= B

    for o in ops:
        assert inside(i, j), (i, j, o)
        if o in "=X":
            assert (o == "=") == (int(db[j]) == int(q[i])), (i, j, o)
            score += M[(int(db[j]) & 31) * 32 + (int(q[i]) & 31)]
            i, j = i + 1, j + 1
        elif o == "D":
            score += extend_gap if prev == "D" else open_gap
            j += 1
        else:
            score += extend_gap if prev == "I" else open_gap
            i += 1
        prev = o
    assert score == int(r["score"]) > 0, (score, int(r["score"]))
    assert ops[0] in "=X" and ops[-1] in "=X"
    if adjacent_gaps_excluded(M, open_gap):
        assert not re.search("ID|DI", ops), ops
    assert i - 1 == int(r["q_end"]) and j - 1 == int(r["s_end"])
    n = {c: ops.count(c) for c in OPS}
    assert n["="] + n["X"] + n["I"] == int(r["q_end"]) - int(r["q_start"]) + 1
    assert n["="] + n["X"] + n["D"] == int(r["s_end"]) - int(r["s_start"]) + 1
    return ops


def within_band(words, q_start, s_start, D, B) -> bool:
    """Whether every cell of a path that starts at (q_start, s_start) lies within B of diagonal D."""
    i, j = q_start, s_start
    for o in expand(words):
        if abs(j - i - D) > B:
            return False
        i, j = i + (o != "D"), j + (o != "I")
    return True


# ---------------------------------------------------------------- unbanded score
def sw_score(q, s, M, open_gap=-11, extend_gap=-1) -> int:
    """The local Smith-Waterman-Gotoh optimum of two short code arrays, in which a
    gap of k letters costs open + (k - 1) * extend."""
    M = [int(x) for x in np.asarray(M).reshape(-1)]
    n, k = len(q), len(s)
    H = [[0] * (k + 1) for _ in range(n + 1)]
    E = [[NEG] * (k + 1) for _ in range(n + 1)]
    F = [[NEG] * (k + 1) for _ in range(n + 1)]
    best = 0
    for a in range(1, n + 1):
        for b in range(1, k + 1):
            E[a][b] = max(E[a][b - 1] + extend_gap, H[a][b - 1] + open_gap)
            F[a][b] = max(F[a - 1][b] + extend_gap, H[a - 1][b] + open_gap)
            H[a][b] = max(0, H[a - 1][b - 1] + M[(int(s[b - 1]) & 31) * 32 + (int(q[a - 1]) & 31)], E[a][b], F[a][b])
            best = max(best, H[a][b])
    return best


# ---------------------------------------------------------------- tile records
def tile_count(m, W, step):
    return len(tc.starts(m, W, step))


def tile_records(seqs, W, step, stride=1):
    """The query chunk of these sources (letter strings) as tile records and one
    BAND_SOURCE record each: stride 1 lays a source's tiles one after the other,
    stride 6 takes the sources six at a time as the frames of one read (they
    must have one length), tile-major and frame-minor. Returns (codes[nrec * W],
    src fields as a list of (first_record, stride, tiles, letters))."""
    recs, src = [], []
    if stride == 1:
        for s in seqs:
            st = tc.starts(len(s), W, step)
            src.append((len(recs), 1, len(st), len(s)))
            recs += [tc.code_record(s[a:a + W], W) for a in st]
    else:
        assert stride == 6 and len(seqs) % 6 == 0
        for g in range(0, len(seqs), 6):
            frames = seqs[g:g + 6]
            assert len({len(f) for f in frames}) == 1
            st = tc.starts(len(frames[0]), W, step)
            base = len(recs)
            for a in st:
                recs += [tc.code_record(f[a:a + W], W) for f in frames]
            src += [(base + f, 6, len(st), len(frames[f])) for f in range(6)]
    return np.concatenate(recs), src


def source_codes(qseq, W, step, src):
    """A source's letters read back through its tile records (the addressing of
    the contract): letter p lies in tile min(p // step, tiles - 1)."""
    first, stride, tiles, m = (int(x) for x in src)
    st = tc.starts(m, W, step)
    assert len(st) == tiles
    out = np.zeros(m, dtype=np.uint8)
    for p in range(m):
        t = min(p // step, tiles - 1)
        out[p] = qseq[(first + (stride * t if tiles > 1 else 0)) * W + p - st[t]]
    return out


# ---------------------------------------------------------------- stage cases
class Case:
    """A stage case: the query chunk's tile records, the DB chunk and the hits."""

    def __init__(self, W, step, stride, B, seqs, subjects, hits, matrix="blosum62", gaps=(-11, -1)):
        from ghostm_amd import BAND_SOURCE_DTYPE

        self.W, self.step, self.stride, self.B, self.matrix, self.gaps = W, step, stride, B, matrix, gaps
        self.seqs = seqs
        self.qseq, src = tile_records(seqs, W, step, stride)
        self.nq = len(self.qseq) // W
        db, self.ranges = [END], []
        for s in subjects:
            self.ranges.append((len(db), len(db) + len(s) - 1))
            db += list(codes(s)) + [END]
        self.db = np.array(db, dtype=np.uint8)
        # hits: (source index, subject index, D relative to the subject's start)
        self.src = np.array([src[q] for q, _, _ in hits], dtype=BAND_SOURCE_DTYPE)
        self.source_of = [q for q, _, _ in hits]
        self.s_lo = np.array([self.ranges[s][0] for _, s, _ in hits], dtype=np.uint32)
        self.s_hi = np.array([self.ranges[s][1] for _, s, _ in hits], dtype=np.uint32)
        self.D = np.array([self.ranges[s][0] + d for _, s, d in hits], dtype=np.int32)

    def M(self):
        import tbext_cases as tx
        return tx.blosum62() if self.matrix == "blosum62" else tx.pam250()

    def sources(self):
        return [codes(self.seqs[q]) for q in self.source_of]

    def host(self, B=None):
        from ghostm_amd import band_align_host
        return band_align_host(self.qseq, self.W, self.db, self.M(), self.src, self.D, self.s_lo, self.s_hi, self.step,
                               self.B if B is None else B, *self.gaps)

    def model(self, B=None):
        return band_model(self.sources(), self.db, self.M(), self.D, self.s_lo, self.s_hi, self.B if B is None else B,
                          *self.gaps)

    def check(self, rec, ops, B=None):
        """The checker on every hit; returns the operation strings."""
        B = self.B if B is None else B
        M = [int(x) for x in np.asarray(self.M()).reshape(-1)]
        return [check_band_path(q, self.db, M, rec[h], hit_words(rec, ops, h), int(self.D[h]), B, int(self.s_lo[h]),
                                int(self.s_hi[h]), *self.gaps) for h, q in enumerate(self.sources())]


def planted(rnd, m, subject, indel=True):
    """A read of m letters (m >= 1): a random flank, a stretch of the subject
    with one planted indel of 1-6 letters copied at an 8 % substitution rate, a
    random flank. Returns (read, read position of the stretch, its subject position)."""
    span = min(rnd.randint(140, 230), len(subject) - 4, max(m - 2, 1))
    s0 = rnd.randint(0, len(subject) - span)
    core = mutate(rnd, subject[s0:s0 + span], 0.08)
    if indel and span > 40:
        p, k = rnd.randint(15, span - 15), rnd.randint(1, 6)
        core = core[:p] + rand_seq(rnd, k) + core[p:] if rnd.random() < 0.5 else core[:p] + core[p + k:]
    core = core[:m]
    q0 = rnd.randint(0, m - len(core))
    read = rand_seq(rnd, q0) + core + rand_seq(rnd, m - q0 - len(core))
    return read, q0, s0


def mixed_case(seed, m, W=127, step=64, stride=1, B=31, n=60, matrix="blosum62", gaps=(-11, -1)):
    """n hits of sources of m letters: planted homologies on their true diagonal
    and shifted off it, bands that overhang s_lo, that overhang s_hi, that cover
    a subject shorter than 2B + 1, and that miss the rectangle altogether."""
    rnd = random.Random(seed * 7919 + m * 31 + W + step + stride + B)
    seqs, subjects, hits = [], [], []
    for h in range(n):
        kind = h % 6
        subj = rand_seq(rnd, rnd.randint(max(40, min(m, 250)), 400))
        read, q0, s0 = planted(rnd, m, subj)
        if kind == 3:  # a subject shorter than the band is wide
            subj = read[:rnd.randint(1, 2 * B)]
            q0 = s0 = 0
        S = len(subj)
        d = s0 - q0
        if kind == 1:
            d += rnd.randint(-B - 2, B + 2)
        elif kind == 2:
            d = rnd.choice([-rnd.randint(0, B), S - 1 - (m - 1) + rnd.randint(0, B)])  # overhangs s_lo / s_hi
        elif kind == 4:
            d = rnd.choice([S + B + rnd.randint(0, 3), -(m - 1) - B - 1 - rnd.randint(0, 3)])  # misses
        elif kind == 5:
            d = rnd.choice([S - 1 + B, -(m - 1) - B])  # touches one corner cell
        seqs.append(read)
        subjects.append(subj)
        hits.append((h, h, d))
    if stride == 6:  # the sources six at a time as one read's frames: all of one length already
        n6 = n - n % 6
        seqs, subjects, hits = seqs[:n6], subjects[:n6], hits[:n6]
    return Case(W, step, stride, B, seqs, subjects, hits, matrix, gaps)


def indel_case(seed, n=40, W=127, step=64, B=31):
    """The issue's prototype inputs: a random flank, a 140-230 residue stretch of
    a random 400 aa subject with one planted indel of 1-6 letters at an 8 %
    substitution rate, a random flank; the anchor is the stretch's first cell."""
    rnd = random.Random(seed)
    seqs, subjects, hits = [], [], []
    for h in range(n):
        subj = rand_seq(rnd, 400)
        read, q0, s0 = planted(rnd, rnd.randint(260, 420), subj)
        seqs.append(read)
        subjects.append(subj)
        hits.append((h, h, s0 - q0))
    return Case(W, step, 1, B, seqs, subjects, hits)


def tie_case(W=127, step=64, B=31, gaps=(-11, -1)):
    """Both sequences one repeated letter, and period-2 repeats: the maximum's
    tie-break, the hsel ties and the open-against-extend ties."""
    seqs, subjects, hits = [], [], []
    for m, S in ((1, 1), (5, 5), (40, 33), (130, 150), (200, 90), (64, 64)):
        for q, s in (("A" * m, "A" * S), ("AW" * (m // 2 + 1), "AW" * (S // 2 + 1)), ("AW" * (m // 2 + 1), "WA" * (S // 2 + 1)),
                     ("A" * m, "AW" * (S // 2 + 1)), ("WC" * (m // 2 + 1), "CCW" * (S // 3 + 1))):
            for d in (0, 1, -3, S - m):
                seqs.append(q[:m])
                subjects.append(s[:S])
                hits.append((len(seqs) - 1, len(subjects) - 1, d))
    return Case(W, step, 1, B, seqs, subjects, hits, gaps=gaps)


def tiny_case(seed, n=60, B=31):
    """m and subject at most 20 and B = 31: the band holds every cell when D is 0."""
    rnd = random.Random(seed)
    seqs, subjects, hits = [], [], []
    for h in range(n):
        subj = rand_seq(rnd, rnd.randint(1, 20))
        k = rnd.randint(1, min(len(subj), 20))
        s0 = rnd.randint(0, len(subj) - k)
        read = mutate(rnd, subj[s0:s0 + k], 0.15)
        if len(read) > 8 and rnd.random() < 0.5:
            p = rnd.randint(3, len(read) - 3)
            read = read[:p] + read[p + 1:]
        read = (rand_seq(rnd, rnd.randint(0, 3)) + read)[:20]
        seqs.append(read)
        subjects.append(subj)
        hits.append((h, h, 0))
    return Case(127, 64, 1, B, seqs, subjects, hits)


W = 127
STEP = 64
# (id, builder): the shapes of the issue. m over the tile boundaries, W = 63 with
# every kind of step, both strides, the three lane counts, the scoring options.
STAGE_CASES = [
    ("m1_B1", lambda: mixed_case(1, 1, B=1)),
    ("m2_B8", lambda: mixed_case(2, 2, B=8)),
    ("mW_B31", lambda: mixed_case(3, W, B=31)),
    ("mW1_B8", lambda: mixed_case(4, W + 1, B=8)),
    ("m2Wstep3_B31", lambda: mixed_case(5, 2 * W + STEP + 3, B=31)),
    ("m2Wstep3_B1", lambda: mixed_case(5, 2 * W + STEP + 3, B=1)),
    ("m1500_B31", lambda: mixed_case(6, 1500, B=31)),
    ("W63_step1", lambda: mixed_case(7, 150, W=63, step=1, B=8)),
    ("W63_step31", lambda: mixed_case(8, 200, W=63, step=31, B=31)),
    ("W63_step62", lambda: mixed_case(9, 190, W=63, step=62, B=31)),
    ("W63_step63", lambda: mixed_case(10, 189, W=63, step=63, B=8)),
    ("stride6", lambda: mixed_case(11, 2 * W + STEP + 3, stride=6, B=31)),
    ("stride6_W63_step31", lambda: mixed_case(12, 140, W=63, step=31, stride=6, B=8)),
    ("pam250_g14e2", lambda: mixed_case(13, 300, B=31, matrix="pam250", gaps=(-14, -2))),
    ("g1e1", lambda: mixed_case(14, 300, B=31, gaps=(-1, -1))),
    ("ties", lambda: tie_case()),
    ("ties_g1e1", lambda: tie_case(gaps=(-1, -1))),
    ("ties_B1", lambda: tie_case(B=1)),
]


# ---------------------------------------------------------------- stage level
def _p(a, t=ctypes.c_uint32):
    return a.ctypes.data_as(ctypes.POINTER(t))


def stage_setup(lib, case):
    """The case's chunks resident through the plugin ABI. The band pass reads no
    k-mer index: an index without positions stands in."""
    from ghostm_amd import native

    M = np.ascontiguousarray(case.M(), dtype=np.int32)
    kc, pos = np.array([0, 1], dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert lib.InitGpu() == 0
    assert lib.SetOptionGpu(1 << 20, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0) == 0, native.last_error()
    assert lib.SetQueryGpu(_p(case.qseq, ctypes.c_uint8), case.nq, case.W) == 0, native.last_error()
    assert lib.SetDbGpu(_p(case.db, ctypes.c_uint8), len(case.db), _p(kc), len(kc), _p(pos), len(pos)) == 0, \
        native.last_error()


def gpu_band(lib, case, B=None, count=None):
    """BandAlignGpu on the resident chunks: the size first (ops == NULL), then the
    words into a buffer with guard words behind them. Returns (rec, ops)."""
    from ghostm_amd import HIT_PATH_DTYPE, native

    n = len(case.src) if count is None else count
    B = case.B if B is None else B
    guard = 0xDEADBEEF
    src, D = np.ascontiguousarray(case.src[:n]), np.ascontiguousarray(case.D[:n])
    lo, hi = np.ascontiguousarray(case.s_lo[:n]), np.ascontiguousarray(case.s_hi[:n])
    rec = np.zeros(n + 1, dtype=HIT_PATH_DTYPE)
    rec["score"][n] = guard

    def call(recp, ops, cap, used):
        return lib.BandAlignGpu(n, src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)), _p(D, ctypes.c_int32),
                                _p(lo), _p(hi), case.W, case.step, B, case.gaps[0], case.gaps[1], recp, ops, cap,
                                ctypes.byref(used))

    used = ctypes.c_size_t(12345)
    assert call(None, None, 0, used) == 0, native.last_error()
    need = used.value
    ops = np.full(need + 4, guard, dtype=np.uint32)
    used2 = ctypes.c_size_t(12345)
    assert call(rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), _p(ops), need, used2) == 0, native.last_error()
    assert used2.value == need
    assert (ops[need:] == guard).all() and rec["score"][n] == guard  # nothing past the last hit's words
    return rec[:n], ops[:need]


def refusal_variants(case):
    """(reason, keyword arguments of a raw call) of every refusal the contract names."""
    def src_with(**kw):
        s = case.src.copy()
        for k, v in kw.items():
            s[k][3] = v
        return s

    lo_bad, hi_bad = case.s_lo.copy(), case.s_hi.copy()
    lo_bad[2] = hi_bad[2] + 1
    hi_over = case.s_hi.copy()
    hi_over[1] = len(case.db)
    return [
        ("source", dict(src=src_with(first_record=case.nq))),
        ("source", dict(src=src_with(tiles=0))),
        ("source", dict(src=src_with(tiles=int(case.src["tiles"][3]) + 1))),
        ("source", dict(src=src_with(letters=int(case.src["letters"][3]) + 200))),
        ("source", dict(step=0)),
        ("source", dict(step=case.W + 1)),
        ("source", dict(nq=int(case.src["first_record"][3]))),
        ("band", dict(B=0)),
        ("band", dict(B=32)),
        ("bounds", dict(lo=lo_bad)),
        ("bounds", dict(hi=hi_over)),
        ("gaps", dict(gaps=(-1, -2))),
        ("gaps", dict(gaps=(-11, 1))),
        ("gaps", dict(gaps=(1, 1))),
        ("ops_cap", dict(ops_cap=3)),
        ("null", dict(used=False)),
    ]


# ---------------------------------------------------------------- session level
def session_inputs(s, W, step=None, dna=False):
    """The band pass's inputs of every hit of a session, rebuilt from what the
    session shows: hits(), hits_path(), hits_rows()["query_record"],
    query_tiles(), query_lengths(), query_records, db_records and db_chunks.
    step None: an untiled set (every record its own single-tile source).
    Returns dict(chunks, dbs, per_hit) with per_hit[h] = (query chunk, DB chunk,
    source fields, tile offset, subject start, subject length, D)."""
    hits = s.hits()
    path, _ = s.hits_path()
    qrec = s.hits_rows()[0]["query_record"]
    tiles, qlen = s.query_tiles(), s.query_lengths()
    assert (len(tiles) > 0) == (step is not None)
    chunks, base, c = [], 0, 0
    while base < len(qlen):
        codes = s.query_records(c)
        chunks.append((base, len(codes) // W, codes))
        base += len(codes) // W
        c += 1
    dbs, dbase = [], 0
    for di, info in enumerate(s.db_chunks()):
        codes = s.db_records(di)
        res = codes != END
        starts = np.flatnonzero(res & np.concatenate([[True], ~res[:-1]]))   # a subject: a maximal run of residues
        ends = np.flatnonzero(res & np.concatenate([~res[1:], [True]]))
        assert len(starts) == info["nseq"]
        dbs.append((dbase, starts, ends - starts + 1, codes))
        dbase += info["nseq"]
    per_hit = []
    for h in range(len(hits)):
        g = int(qrec[h])
        qi = max(k for k, ch in enumerate(chunks) if ch[0] <= g)
        local = g - chunks[qi][0]
        if step is None:
            src, offset = (local, 1, 1, int(qlen[g])), 0
        else:
            t = tiles[g]
            m, offset = max(int(t["letters"]), 1), int(t["offset"])
            st = tc.starts(m, W, step)
            stride = 6 if dna else 1
            src = (local - st.index(offset) * stride, stride, len(st), m)
        di = max(k for k, d in enumerate(dbs) if d[0] <= int(hits["db_id"][h]))
        subj = int(hits["db_id"][h]) - dbs[di][0]
        pos, length = int(dbs[di][1][subj]), int(dbs[di][2][subj])
        D = pos + int(path["s_start"][h]) - (offset + int(path["q_start"][h]))
        per_hit.append((qi, di, src, offset, pos, length, D))
    return dict(chunks=chunks, dbs=dbs, per_hit=per_hit)


def session_expected(inp, W, step, band, M, gaps=(-11, -1)):
    """The host model's (records, ops) of every session hit from session_inputs:
    one call per (query chunk, DB chunk), subject coordinates relative to the
    subject, the words in hit order. Returns (rec, ops, calls)."""
    from ghostm_amd import BAND_SOURCE_DTYPE, HIT_PATH_DTYPE, band_align_host

    per_hit = inp["per_hit"]
    want = np.zeros(len(per_hit), dtype=HIT_PATH_DTYPE)
    words = [None] * len(per_hit)
    groups = {}
    for h, x in enumerate(per_hit):
        groups.setdefault((x[0], x[1]), []).append(h)
    for (qi, di), idx in groups.items():
        src = np.array([per_hit[h][2] for h in idx], dtype=BAND_SOURCE_DTYPE)
        lo = [per_hit[h][4] for h in idx]
        hi = [per_hit[h][4] + per_hit[h][5] - 1 for h in idx]
        rec, ops = band_align_host(inp["chunks"][qi][2], W, inp["dbs"][di][3], M, src, [per_hit[h][6] for h in idx], lo,
                                   hi, step or W, band, *gaps)
        for k, h in enumerate(idx):
            want[h] = rec[k]
            want["s_start"][h] -= lo[k]
            want["s_end"][h] -= lo[k]
            words[h] = hit_words(rec, ops, k)
    at = 0
    for h in range(len(per_hit)):
        want["ops_offset"][h] = at
        at += len(words[h])
    all_ops = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, dtype=np.uint32)
    return want, all_ops, len(groups)


def check_session(inp, W, step, band, M, rec, ops, gaps=(-11, -1)):
    """The checker on every session hit; returns the operation strings."""
    Ml = [int(x) for x in np.asarray(M).reshape(-1)]
    out = []
    for h, (qi, di, src, offset, pos, length, D) in enumerate(inp["per_hit"]):
        q = source_codes(inp["chunks"][qi][2], W, step or W, src)
        r = dict(q_start=rec["q_start"][h], q_end=rec["q_end"][h], s_start=int(rec["s_start"][h]) + pos,
                 s_end=int(rec["s_end"][h]) + pos, score=rec["score"][h], n_runs=rec["n_runs"][h])
        out.append(check_band_path(q, inp["dbs"][di][3], Ml, r, hit_words(rec, ops, h), D, band, pos, pos + length - 1,
                                   *gaps))
    return out
