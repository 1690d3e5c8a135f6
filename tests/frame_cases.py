"""Shared by tests/test_frame_align_host.py, tests/test_gpu_frame_align.py and
tests/frame_poison_child.py (not a test module): a Python model of the
frameshift-aware read-level alignment written from its contract, the checker
that re-walks a path along the sequences, the builders of reads with planted
single-nucleotide indels and the stage cases.

The contract (include/ghostm_hip.h, FrameAlignGpu). Per hit: one strand of a
DNA read as three frames g = 0, 1, 2 of m letters, strand position p = 3c + g
with letter q(p) = letter p // 3 of frame p % 3; a subject range [s_lo, s_hi];
an anchor diagonal D; a half-width B. The band cells are (p, j) with 0 <= p <
3m, s_lo <= j <= s_hi, |j - p // 3 - D| <= B. Reverse DP, rows p = 3m-1..0, j
descending in a row, all int32:
    d0 = H(p+3,j+1); d1 = H(p+2,j+1) + shift; d2 = H(p+4,j+1) + shift
    diag, fsel = d0, 0; d1 > diag: d1, 1; d2 > diag: d2, 2
    s      = diag + M[db[j]*32 + q(p)]
    E(p,j) = max(E(p,j+1) + ext, H(p,j+1) + open)     'D'
    F(p,j) = max(F(p+3,j) + ext, H(p+3,j) + open)     'I'
    H(p,j) = s if s > 0 else 0; then E if E > H; then F if F > H (hsel 0/1/2/3)
    eext   = E(p,j+1) + ext > H(p,j+1) + open (a tie opens); fext likewise
A neighbour that is no band cell has H = 0 and E = F = minus infinity. The
start cell is the first strict maximum in processing order; the walk:
    H, hsel 1   emit '=' / 'X'; fsel 1: emit '/' and go to (p+2, j+1); fsel 2:
                emit '\\' and go to (p+4, j+1); else go to (p+3, j+1)
    H, hsel 2/3 enter E / F at the same cell
    H, hsel 0   stop; leaving the band cells stops
    E           emit 'D', go to E(p, j+1) if eext else H(p, j+1)
    F           emit 'I', go to F(p+3, j) if fext else H(p+3, j)
Score 0: an empty path at q_start = 0, s_start = s_lo."""
from __future__ import annotations

import ctypes
import itertools
import random

import numpy as np

import band_cases as bc
import tile_cases as tc

END = 25
OPS = "=XID\\/"      # op codes 0..5: 4 is the late shift, 5 the early one
NEG = -(1 << 29)
NO_SHIFT = -(1 << 20)
W = 127
STEP = 64

# residues whose codon below has no T in its second or third base: no frame of a
# back-translated stretch holds a stop codon or an ATG, whatever follows what
ALPHA = "ARNDCQEGHKPSTWY"
CODON = dict(A="GCC", R="CGC", N="AAC", D="GAC", C="TGC", Q="CAG", E="GAG", G="GGC", H="CAC", K="AAG", P="CCC",
             S="AGC", T="ACC", W="TGG", Y="TAC")


# ---------------------------------------------------------------- small helpers
def codes(s: str) -> np.ndarray:
    return np.array([tc.ORDER.index(c) for c in s], dtype=np.uint8)


def rand_prot(rnd, n: int) -> str:
    return "".join(rnd.choice(ALPHA) for _ in range(n))


def back_translate(prot: str) -> str:
    return "".join(CODON[c] for c in prot)


def translate(dna: str, o: int, m: int) -> str:
    """m letters of the frame at offset o: letter t is the codon at strand
    positions o + 3t .. o + 3t + 2, '*' where the codon is not whole."""
    out = []
    for t in range(m):
        k = o + 3 * t
        out.append(tc.CODONS[int("".join(str("ACGT".index(b)) for b in dna[k:k + 3]), 4)] if k + 3 <= len(dna) else "*")
    return "".join(out)


def strand_frames(dna: str) -> tuple:
    """The three frames of a strand, len(dna) // 3 letters each (at least 1)."""
    m = max(len(dna) // 3, 1)
    return tuple(translate(dna, o, m) for o in range(3))


def runs(ops: str) -> list:
    return [len(list(g)) << 4 | OPS.index(c) for c, g in itertools.groupby(ops)]


def expand(words) -> str:
    return "".join(OPS[int(w) & 15] * (int(w) >> 4) for w in words)


hit_words = bc.hit_words


# ---------------------------------------------------------------- Python model
def frame_model(frames, db, M, D, s_lo, s_hi, B, open_gap=-11, extend_gap=-1, shift=-15):
    """All hits of a case at once (numpy over the hits; the rows and the E chain
    of a row run one after the other, as the recurrence says). frames: per hit
    three code arrays of one length. A neighbour is looked up by its
    coordinates: the lane of (p', j') is j' - p' // 3 - D + B. Returns a list of
    dict(score, q_start, q_end, s_start, s_end, ops)."""
    n, lanes = len(frames), 2 * B + 1
    m = np.array([len(f[0]) for f in frames], dtype=np.int64)
    P = int(3 * m.max())
    Q = np.zeros((n, P), dtype=np.int64)
    for h, f in enumerate(frames):
        for g in range(3):
            Q[h, g:3 * len(f[g]):3] = np.asarray(f[g], dtype=np.int64) & 31
    db = np.asarray(db, dtype=np.int64)
    M2 = np.asarray(M, dtype=np.int64).reshape(32, 32)
    D = np.asarray(D, dtype=np.int64)
    lo = np.asarray(s_lo, dtype=np.int64)
    hi = np.asarray(s_hi, dtype=np.int64)
    lane = np.arange(lanes, dtype=np.int64)
    H = np.zeros((P + 5, n, lanes), dtype=np.int64)     # rows at and past 3m: no band cells
    F = np.full((P + 5, n, lanes), NEG, dtype=np.int64)
    dirs = np.zeros((P, n, lanes), dtype=np.uint8)
    best = np.zeros(n, dtype=np.int64)
    bp = np.zeros(n, dtype=np.int64)
    bj = lo.copy()

    def at(A, p, p2, dj, fill):
        """A at (p2, j + dj) for every lane's j of row p; fill where that is no lane."""
        d = dj - (p2 // 3 - p // 3)
        out = np.full((n, lanes), fill, dtype=np.int64)
        if d == 0:
            out[:] = A[p2]
        elif 0 < d < lanes:
            out[:, :-d] = A[p2][:, d:]
        elif -lanes < d < 0:
            out[:, -d:] = A[p2][:, :d]
        return out

    for p in range(P - 1, -1, -1):
        j = p // 3 + D[:, None] - B + lane[None, :]
        cell_ok = (p < 3 * m)[:, None] & (j >= lo[:, None]) & (j <= hi[:, None])
        sub = M2[db[np.clip(j, 0, len(db) - 1)] & 31, Q[:, p][:, None]]
        diag = at(H, p, p + 3, 1, 0)
        fsel = np.zeros((n, lanes), dtype=np.int64)
        for k, p2 in ((1, p + 2), (2, p + 4)):
            d = at(H, p, p2, 1, 0) + shift
            t = d > diag
            diag, fsel = np.where(t, d, diag), np.where(t, k, fsel)
        s = diag + sub
        fe, fo = at(F, p, p + 3, 0, NEG) + extend_gap, at(H, p, p + 3, 0, 0) + open_gap
        Fn = np.maximum(fe, fo)
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
            t = Fn[:, b] > cell
            cell, sel = np.where(t, Fn[:, b], cell), np.where(t, 3, sel)
            ok = cell_ok[:, b]
            Hc[:, b] = np.where(ok, cell, 0)
            Ec[:, b] = np.where(ok, E, NEG)
            dirs[p, :, b] = np.where(ok, sel | (ee > eo) << 2 | (fe[:, b] > fo[:, b]) << 3 | fsel[:, b] << 5, 0)
        Hrow = Hc[:, :lanes]
        rowmax = Hrow.max(axis=1)
        arg = lanes - 1 - np.argmax(Hrow[:, ::-1] == rowmax[:, None], axis=1)   # j descends: the largest lane first
        upd = rowmax > best
        best = np.where(upd, rowmax, best)
        bp = np.where(upd, p, bp)
        bj = np.where(upd, p // 3 + D - B + arg, bj)
        H[p] = Hrow
        F[p] = np.where(cell_ok, Fn, NEG)

    out = []
    for h in range(n):
        p, j, state, ops = int(bp[h]), int(bj[h]), "H", []

        def cell(p, j):
            b = j - p // 3 - int(D[h]) + B
            if p >= 3 * m[h] or j > hi[h] or j < lo[h] or b < 0 or b >= lanes:
                return None
            return int(dirs[p, h, b])

        if best[h] > 0:
            while True:
                d = cell(p, j)
                if d is None:
                    break
                if state == "H":
                    if d & 3 == 0:
                        break
                    if d & 3 == 1:
                        ops.append("=" if int(db[j]) & 31 == int(Q[h, p]) else "X")
                        fs = d >> 5 & 3
                        if fs:
                            ops.append("/" if fs == 1 else "\\")
                        p, j = p + (3, 2, 4)[fs], j + 1
                    else:
                        state = "E" if d & 3 == 2 else "F"
                elif state == "E":
                    ops.append("D")
                    state = "E" if d & 4 else "H"
                    j += 1
                else:
                    ops.append("I")
                    state = "F" if d & 8 else "H"
                    p += 3
        out.append(dict(score=int(best[h]), q_start=int(bp[h]), s_start=int(bj[h]),
                        q_end=p - 1 if best[h] > 0 else int(bp[h]), s_end=j - 1 if best[h] > 0 else int(bj[h]),
                        ops="".join(ops)))
    return out


def assert_equals_model(rec, ops, model):
    """(rec, ops) of a host or device call against frame_model's list."""
    assert len(rec) == len(model)
    for h, r in enumerate(model):
        got = tuple(int(rec[f][h]) for f in ("q_start", "q_end", "s_start", "s_end", "score"))
        assert got == (r["q_start"], r["q_end"], r["s_start"], r["s_end"], r["score"]), (h, got, r)
        assert list(hit_words(rec, ops, h)) == runs(r["ops"]), (h, r["ops"])
    n_runs = np.asarray(rec["n_runs"], dtype=np.int64)
    assert np.array_equal(rec["ops_offset"], np.concatenate([[0], np.cumsum(n_runs)[:-1]]).astype(np.uint64))
    assert len(ops) == int(n_runs.sum())


# ---------------------------------------------------------------- the checker
def check_frame_path(frames, db, M, r, words, D, B, s_lo, s_hi, open_gap, extend_gap, shift):
    """Re-walks one hit's path along the sequences: '=' / 'X' consume 3 nt and a
    residue, '\\' one nt more, '/' one nt less, 'I' 3 nt, 'D' a residue. The
    rescore equals the score, every cell the path emits at lies inside the band
    cells, q_end and s_end match, no path starts or ends with a shift and no two
    shifts are adjacent. Returns the operation string."""
    M = M if isinstance(M, list) else [int(x) for x in np.asarray(M).reshape(-1)]
    m = len(frames[0])
    assert int(r["n_runs"]) == len(words)
    if int(r["score"]) == 0:
        assert len(words) == 0 and int(r["q_end"]) == int(r["q_start"]) == 0
        assert int(r["s_end"]) == int(r["s_start"]) == s_lo
        return ""
    for a, b in zip(words[:-1], words[1:]):
        assert (int(a) & 15) != (int(b) & 15)  # maximal runs
    assert all(int(w) & 15 <= 5 and int(w) >> 4 > 0 for w in words)
    ops = expand(words)
    p, j, score, prev = int(r["q_start"]), int(r["s_start"]), 0, None

    def inside(p, j):
        return 0 <= p < 3 * m and s_lo <= j <= s_hi and abs(j - p // 3 - D) <= B

    for o in ops:
        if o in "=X":
            assert inside(p, j), (p, j, o)
            q = int(frames[p % 3][p // 3]) & 31
            assert (o == "=") == (int(db[j]) & 31 == q), (p, j, o)
            score += M[(int(db[j]) & 31) * 32 + q]
            p, j = p + 3, j + 1
        elif o in "\\/":
            assert prev in ("=", "X"), ops    # a shift follows a pair: none first, no two adjacent
            score += shift
            p += 1 if o == "\\" else -1
        elif o == "D":
            assert inside(p, j), (p, j, o)
            score += extend_gap if prev == "D" else open_gap
            j += 1
        else:
            assert inside(p, j), (p, j, o)
            score += extend_gap if prev == "I" else open_gap
            p += 3
        prev = o
    assert score == int(r["score"]) > 0, (score, int(r["score"]), ops)
    assert ops[0] in "=X" and ops[-1] in "=X", ops
    assert p - 1 == int(r["q_end"]) and j - 1 == int(r["s_end"])
    return ops


# ---------------------------------------------------------------- stage cases
class Case:
    """A stage case: reads as six frame strings each (frames 0-2 strand 0, 3-5
    strand 1; one length per read), laid out tile-major and frame-minor, the DB
    chunk and the hits (read, strand, subject, D relative to the subject's
    start, residues cut off the subject's range on the left and right)."""

    def __init__(self, B, reads, subjects, hits, W=W, step=STEP, gaps=(-11, -1), shift=-15, one_tile_stride=6):
        from ghostm_amd import BAND_SOURCE_DTYPE

        self.W, self.step, self.B, self.gaps, self.shift = W, step, B, gaps, shift
        self.reads = reads
        self.qseq, src6 = bc.tile_records([f for r in reads for f in r], W, step, 6)
        # a one-tile source's stride is not read: any value will do
        self.src6 = [(f, s if t > 1 else one_tile_stride, t, m) for f, s, t, m in src6]
        self.nq = len(self.qseq) // W
        db, self.ranges = [END], []
        for s in subjects:
            self.ranges.append((len(db), len(db) + len(s) - 1))
            db += list(codes(s)) + [END]
        self.db = np.array(db, dtype=np.uint8)
        self.strand_of = [(r, s) for r, s, _, _, _, _ in hits]
        self.src = np.array([self.src6[6 * r + 3 * s] for r, s in self.strand_of], dtype=BAND_SOURCE_DTYPE)
        self.s_lo = np.array([self.ranges[s][0] + a for _, _, s, _, a, _ in hits], dtype=np.uint32)
        self.s_hi = np.array([self.ranges[s][1] - b for _, _, s, _, _, b in hits], dtype=np.uint32)
        self.D = np.array([self.ranges[s][0] + d for _, _, s, d, _, _ in hits], dtype=np.int32)

    def M(self):
        import tbext_cases as tx
        return tx.blosum62()

    def frames(self):
        return [tuple(codes(f) for f in self.reads[r][3 * s:3 * s + 3]) for r, s in self.strand_of]

    def host(self, shift=None, B=None):
        from ghostm_amd import frame_align_host
        return frame_align_host(self.qseq, self.W, self.db, self.M(), self.src, self.D, self.s_lo, self.s_hi, self.step,
                                self.B if B is None else B, *self.gaps, self.shift if shift is None else shift)

    def band_host(self, g):
        """GhostmBandAlignHost on frame g of every hit's strand, same D, B and range."""
        from ghostm_amd import BAND_SOURCE_DTYPE, band_align_host
        src = np.array([self.src6[6 * r + 3 * s + g] for r, s in self.strand_of], dtype=BAND_SOURCE_DTYPE)
        return band_align_host(self.qseq, self.W, self.db, self.M(), src, self.D, self.s_lo, self.s_hi, self.step,
                               self.B, *self.gaps)

    def model(self, shift=None):
        return frame_model(self.frames(), self.db, self.M(), self.D, self.s_lo, self.s_hi, self.B, *self.gaps,
                           self.shift if shift is None else shift)

    def check(self, rec, ops, shift=None):
        M = [int(x) for x in np.asarray(self.M()).reshape(-1)]
        return [check_frame_path(f, self.db, M, rec[h], hit_words(rec, ops, h), int(self.D[h]), self.B,
                                 int(self.s_lo[h]), int(self.s_hi[h]), *self.gaps, self.shift if shift is None else shift)
                for h, f in enumerate(self.frames())]


def mutate(rnd, s: str, rate: float) -> str:
    return "".join(rnd.choice(ALPHA) if rnd.random() < rate else c for c in s)


def planted_read(rnd, nt, subject, indels, prefix=None):
    """A strand of nt nucleotides: a flank, a stretch of the subject
    back-translated at a 6 % substitution rate with `indels` single-nucleotide
    insertions or deletions planted in it, a flank. prefix: the nucleotides
    before the stretch (None: random). Returns (dna, strand position of the
    stretch, its subject position)."""
    span = min(rnd.randint(40, 90), len(subject), max(nt // 3 - 1, 1))
    s0 = rnd.randint(0, len(subject) - span)
    core = back_translate(mutate(rnd, subject[s0:s0 + span], 0.06))
    for _ in range(indels):
        if len(core) < 40:
            break
        at = rnd.randint(12, len(core) - 12)
        core = core[:at] + rnd.choice("CG") + core[at:] if rnd.random() < 0.5 else core[:at] + core[at + 1:]
    core = core[:nt]
    q0 = rnd.randint(0, nt - len(core)) if prefix is None else min(prefix, nt - len(core))
    flank = back_translate(rand_prot(rnd, nt // 3 + 2))
    dna = flank[:q0] + core + flank[q0:q0 + nt - q0 - len(core)]
    assert len(dna) == nt
    return dna, q0, s0


def mixed_case(seed, m, B, W=W, step=STEP, n=18, shift=-15, gaps=(-11, -1), one_tile_stride=6):
    """n hits on strands of 3m .. 3m+2 nucleotides (m letters a frame): planted
    homologies with up to two single-nucleotide indels, anchored on the true
    diagonal of their first codon and off it; D negative and past the subject;
    ranges cut inside the subject on both sides; bands that miss the range."""
    rnd = random.Random(seed * 7919 + m * 31 + W + step + B)
    reads, subjects, hits = [], [], []
    for h in range(n):
        kind = (h + 3) % 6
        subj = rand_prot(rnd, rnd.randint(max(30, min(m, 120)), 220))
        nt = 3 * m + rnd.randint(0, 2)
        dna, q0, s0 = planted_read(rnd, nt, subj, indels=h % 3)
        other, _, _ = planted_read(rnd, nt, subj, indels=1)
        strand = h % 2
        frames = strand_frames(other) + strand_frames(dna) if strand else strand_frames(dna) + strand_frames(other)
        S = len(subj)
        d, cut_lo, cut_hi = s0 - q0 // 3, 0, 0
        if kind == 1:
            d += rnd.randint(-B - 2, B + 2)
        elif kind == 2:    # the range cuts the band on both sides
            cut_lo, cut_hi = min(s0 + rnd.randint(1, 8), S - 2), min(rnd.randint(1, 8), S - 2)
            if cut_lo + cut_hi >= S:
                cut_lo, cut_hi = 0, 0
        elif kind == 3:    # D negative (the first subject's hit), D past the subject's end; a corner met or not
            d = -rnd.randint(2, m + B + 2) if h == 0 else S - 1 + rnd.randint(1, B + 2)
        elif kind == 4:    # overhangs s_lo / s_hi
            d = rnd.choice([-rnd.randint(0, B), S - 1 - (m - 1) + rnd.randint(0, B)])
        reads.append(frames)
        subjects.append(subj)
        hits.append((h, strand, h, d, cut_lo, cut_hi))
    return Case(B, reads, subjects, hits, W=W, step=step, gaps=gaps, shift=shift, one_tile_stride=one_tile_stride)


def truth_case(seed, kind, B=3):
    """The planted truth: a subject stretch of 60 residues back-translated with
    one fixed codon per residue, one nucleotide inserted after codon 30 ('ins')
    or the first nucleotide of codon 30 deleted ('del'); the read is the stretch
    alone, the subject the stretch between two flanks. Returns (case, position
    of the stretch in the subject)."""
    rnd = random.Random(seed)
    stretch = rand_prot(rnd, 60)
    left, right = rand_prot(rnd, 17), rand_prot(rnd, 23)
    dna = back_translate(stretch)
    dna = dna[:90] + "G" + dna[90:] if kind == "ins" else dna[:90] + dna[91:]
    frames = strand_frames(dna) + strand_frames(back_translate(rand_prot(rnd, len(dna) // 3 + 1))[:len(dna)])
    return Case(B, [frames], [left + stretch + right], [(0, 0, 0, len(left), 0, 0)]), len(left)


def lane_edge_case(kind, B, b, seed=5):
    """A planted shift whose source cell lies on a chosen lane. kind 'early':
    the pairs before the shift are at g = 0 on lane b and the '/' steps to row
    p + 2 of the same codon, lane b + 1 (b = 2B: no cell). kind 'late': the
    pairs before are at g = 2 on lane b and the '\\' steps to row p + 4, two
    codons up, lane b - 1 (b = 0: no cell)."""
    rnd = random.Random(seed * 131 + B * 7 + b)
    stretch = rand_prot(rnd, 50)
    left, right = rand_prot(rnd, 2 * B + 5), rand_prot(rnd, 2 * B + 5)
    dna = back_translate(stretch)
    if kind == "early":   # codons 0..24 at g = 0, then one nucleotide of codon 25 missing
        dna = dna[:75] + dna[76:]
    else:                 # two nucleotides in front: codons 0..24 at g = 2, then one inserted
        dna = "GC" + dna[:75] + "C" + dna[75:]
    frames = strand_frames(dna) + strand_frames(back_translate(rand_prot(rnd, len(dna) // 3 + 1))[:len(dna)])
    # lane of the first segment: j - c = len(left) relative to the subject, so D = len(left) - b + B
    return Case(B, [frames], [left + stretch + right], [(0, 0, 0, len(left) - b + B, 0, 0)])


def many_rows_case(seed=9, n=11, B=8):
    """Hits of different row counts (reads of 20 to 260 letters a frame), a count
    that is no multiple of the waves of a block."""
    rnd = random.Random(seed)
    reads, subjects, hits = [], [], []
    for h in range(n):
        m = rnd.choice([20, 40, 90, 127, 128, 200, 260])
        subj = rand_prot(rnd, rnd.randint(60, 200))
        dna, q0, s0 = planted_read(rnd, 3 * m + h % 3, subj, indels=1 + h % 2)
        other, _, _ = planted_read(rnd, 3 * m + h % 3, subj, indels=0)
        reads.append(strand_frames(dna) + strand_frames(other))
        subjects.append(subj)
        hits.append((h, 0, h, s0 - q0 // 3, 0, 0))
    return Case(B, reads, subjects, hits)


# (id, builder): B over the three lane counts, m over the tile boundaries, 1, 2
# and 3 tiles with the flush-right last one, the three steps, a one-tile source
# with a stride that must not be read
STAGE_CASES = [
    ("m1_B1", lambda: mixed_case(1, 1, 1, one_tile_stride=0)),
    ("m2_B2", lambda: mixed_case(2, 2, 2)),
    ("m3_B31", lambda: mixed_case(3, 3, 31, one_tile_stride=12345)),
    ("m127_B31", lambda: mixed_case(4, 127, 31, n=12)),
    ("m127_B1", lambda: mixed_case(5, 127, 1, one_tile_stride=0)),
    ("m128_B2_two_tiles", lambda: mixed_case(6, 128, 2)),
    ("m128_step1_B31", lambda: mixed_case(7, 128, 31, step=1, n=12)),
    ("m129_step1_three_tiles", lambda: mixed_case(8, 129, 2, step=1)),
    ("m200_B31_three_tiles", lambda: mixed_case(9, 200, 31, n=12)),
    ("m200_B2", lambda: mixed_case(10, 200, 2)),
    ("m203_step127_B1", lambda: mixed_case(11, 203, 1, step=127)),
    ("m254_step127_B2", lambda: mixed_case(12, 254, 2, step=127, n=12)),
    ("g1e1_shift0", lambda: mixed_case(13, 150, 2, gaps=(-1, -1), shift=0)),
    ("shift_3", lambda: mixed_case(14, 150, 31, shift=-3, n=12)),
    ("rows", lambda: many_rows_case()),
]
LANE_CASES = [(kind, B, b) for kind, B, bs in (("early", 3, (5, 6)), ("late", 3, (1, 0)), ("early", 31, (61, 62)),
                                               ("late", 31, (1, 0)), ("early", 1, (1, 2)), ("late", 1, (1, 0)))
              for b in bs]


# ---------------------------------------------------------------- stage level
_p = bc._p
stage_setup = bc.stage_setup


def gpu_frame(lib, case, shift=None, count=None):
    """FrameAlignGpu on the resident chunks: the size first (ops == NULL), then
    the words into a buffer with guard words behind them. Returns (rec, ops)."""
    from ghostm_amd import HIT_PATH_DTYPE, native

    n = len(case.src) if count is None else count
    shift = case.shift if shift is None else shift
    guard = 0xDEADBEEF
    src, D = np.ascontiguousarray(case.src[:n]), np.ascontiguousarray(case.D[:n])
    lo, hi = np.ascontiguousarray(case.s_lo[:n]), np.ascontiguousarray(case.s_hi[:n])
    rec = np.zeros(n + 1, dtype=HIT_PATH_DTYPE)
    rec["score"][n] = guard

    def call(recp, ops, cap, used):
        return lib.FrameAlignGpu(n, src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)), _p(D, ctypes.c_int32),
                                 _p(lo), _p(hi), case.W, case.step, case.B, case.gaps[0], case.gaps[1], shift, recp,
                                 ops, cap, ctypes.byref(used))

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
    out = bc.refusal_variants(case)
    # the strand's frame 2 of the last tile must lie in the chunk: frame 0's alone does not do
    last = int(case.src["first_record"][3]) + (int(case.src["tiles"][3]) - 1) * 6
    return out + [("source", dict(nq=last + 2)), ("shift", dict(shift=1)), ("shift", dict(shift=-(1 << 20) - 1))]
