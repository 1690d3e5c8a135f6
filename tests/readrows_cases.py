"""Shared by tests/test_read_rows_host.py, tests/test_gpu_read_rows.py and
tests/readrows_poison_child.py (not a test module): a Python model of the
read-level aligned rows written from their contract, the hand-made path sets
and the sets made of the band and frame passes' own paths.

The contract (include/ghostm_hip.h, GhostmHitReadRows / ReadRowsGpu). Per hit: a
source (first_record, stride, tiles, letters), W and step; a path (q_start,
s_start absolute in the chunk, words length << 4 | op). Letter c of frame offset
g lies in tile t = min(c // step, tiles - 1), whose start is t * step, or
max(letters - W, 0) for the last tile; its record is first_record + g + stride
* t (stride unread when tiles == 1), its byte c - start(t). Every word gives
its length in columns. Band mode: a column of op 0, 1, 2 shows the letter at the
position and advances it by 1. Frame mode: the position p is in nucleotides; a
column of op 0, 1, 2 shows letter p // 3 of frame p % 3 and advances p by 3, a
column of op 4 ('\\') advances p by 1, one of op 5 ('/') takes 1 from it. Ops 0,
1, 3 advance the subject by 1. Text: the letter table, '?' from code 25 up; the
midline is the query letter on '=', '+' on an 'X' whose M[(db & 31) * 32 +
(query & 31)] is > 0, a space otherwise; a shift column is '\\' or '/', a
space, '-'. Counts: identities ('=' columns), positives (pair columns with M >
0), gap_residues ('I' and 'D' columns), shifts (columns of ops 4 and 5); the
rescore is the pair columns' M plus open for the first and ext for every
further column of an 'I' or 'D' word plus shift_cost per shift column.
query_record is the record of the letter at q_start; first_record for a path
without words."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import band_cases as bc
import frame_cases as fc
import tile_cases as tc

LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"
OPS = "=XID\\/"
END = 25
W, STEP = 127, 64


def letter(c: int) -> str:
    return LETTERS[c] if c < 25 else "?"


def locate(src, g, c, W, step):
    """(record, byte) of letter c of frame offset g of a source."""
    first, stride, tiles, m = (int(x) for x in src)
    t = min(c // step, tiles - 1)
    start = t * step if t < tiles - 1 else max(m - W, 0)
    return first + g + (stride * t if tiles > 1 else 0), c - start


# ---------------------------------------------------------------- Python model
def rows_model(qseq, W, step, db, M, src, rec, ops, frame, open_gap=-11, extend_gap=-1, shift_cost=-15):
    """The contract, column by column. Returns (records[READ_ROWS_DTYPE], rows[uint8])."""
    from ghostm_amd import READ_ROWS_DTYPE

    M = [int(x) for x in np.asarray(M).reshape(-1)]
    out = np.zeros(len(rec), dtype=READ_ROWS_DTYPE)
    text = []
    at = 0
    for h in range(len(rec)):
        words = [int(w) for w in bc.hit_words(rec, ops, h)]
        p, s = int(rec["q_start"][h]), int(rec["s_start"][h])
        qrow, mid, srow = [], [], []
        ident = posit = gaps = shifts = score = 0

        def query_code():
            r, b = locate(src[h], p % 3, p // 3, W, step) if frame else locate(src[h], 0, p, W, step)
            return int(qseq[r * W + b])

        first_record = int(src[h]["first_record"])
        if words:
            first_record = (locate(src[h], p % 3, p // 3, W, step) if frame else locate(src[h], 0, p, W, step))[0]
        for w in words:
            op, n = w & 15, w >> 4
            for k in range(n):
                if op < 2:
                    qc, sc = query_code(), int(db[s])
                    m = M[(sc & 31) * 32 + (qc & 31)]
                    qrow.append(letter(qc))
                    srow.append(letter(sc))
                    mid.append(letter(qc) if op == 0 else "+" if m > 0 else " ")
                    score += m
                    posit += m > 0
                    ident += op == 0
                elif op == 2:
                    qrow.append(letter(query_code()))
                    mid.append(" ")
                    srow.append("-")
                elif op == 3:
                    qrow.append("-")
                    mid.append(" ")
                    srow.append(letter(int(db[s])))
                else:
                    qrow.append(OPS[op])
                    mid.append(" ")
                    srow.append("-")
                if op in (2, 3):
                    gaps += 1
                    score += open_gap if k == 0 else extend_gap
                if op >= 4:
                    shifts += 1
                    score += shift_cost
                if op <= 2:
                    p += 3 if frame else 1
                elif op == 4:
                    p += 1
                elif op == 5:
                    p -= 1
                if op in (0, 1, 3):
                    s += 1
        n = len(qrow)
        out[h] = (first_record, n, ident, posit, gaps, score, at, shifts, 0)
        text.append("".join(qrow) + "".join(mid) + "".join(srow))
        at += 3 * n
    rows = np.frombuffer("".join(text).encode("latin-1"), dtype=np.uint8).copy()
    return out, rows


# ---------------------------------------------------------------- path sets
class RowSet:
    """The inputs of one rows call: the query chunk's records, the DB chunk, the
    hits' sources and paths. frame: 0 band paths, 1 frame paths."""

    def __init__(self, qseq, W, step, db, matrix, src, rec, ops, frame, gaps=(-11, -1), shift=-15):
        from ghostm_amd import BAND_SOURCE_DTYPE, HIT_PATH_DTYPE

        self.qseq, self.W, self.step, self.db, self.matrix = np.ascontiguousarray(qseq, dtype=np.uint8), W, step, db, matrix
        self.nq = len(self.qseq) // W
        self.src = np.ascontiguousarray(src, dtype=BAND_SOURCE_DTYPE)
        self.rec = np.ascontiguousarray(rec, dtype=HIT_PATH_DTYPE)
        self.ops = np.ascontiguousarray(ops, dtype=np.uint32)
        self.frame, self.gaps, self.shift = frame, gaps, shift

    def M(self):
        return self.matrix

    def model(self):
        return rows_model(self.qseq, self.W, self.step, self.db, self.matrix, self.src, self.rec, self.ops, self.frame,
                          *self.gaps, self.shift)

    def host(self, count=None):
        from ghostm_amd import read_rows_host
        n = len(self.src) if count is None else count
        return read_rows_host(self.qseq, self.W, self.db, self.matrix, self.src[:n], self.rec[:n], self.ops, self.step,
                              self.frame, *self.gaps, self.shift)


def _paths(paths):
    """(rec, ops) of [(q_start, s_start, words)]: the words one after the other."""
    from ghostm_amd import HIT_PATH_DTYPE

    rec = np.zeros(len(paths), dtype=HIT_PATH_DTYPE)
    ops = []
    for h, (q0, s0, words) in enumerate(paths):
        rec[h] = (q0, 0, s0, 0, 0, len(words), len(ops))
        ops += list(words)
    return rec, np.array(ops, dtype=np.uint32)


def _db(rnd, n):
    """END, n residues, END; codes 25..31 and 25 at 40..46 (never an END to a rows call)."""
    db = np.array([END] + [rnd.randrange(20) for _ in range(n)] + [END], dtype=np.uint8)
    db[40:47] = [26, 27, 28, 29, 30, 31, 25]
    return db


def hand_band_set():
    """Source A: 200 letters at W = 127, step 64, three tiles, the last starting
    at 73. Source B: one tile of 5 letters. Source C: one tile of the codes 25..31.
    Paths: one '=' run of 200 columns (both tile starts, the flush-right
    overlap, 4 column groups); 130 words of length 1 alternating '=', 'I', 'D'
    (three word groups with carries); an empty path; the 5 letters; the codes
    25..31 against subject codes 26..31 and 25 ('?' and the five-bit index)."""
    import tbext_cases as tx

    rnd = random.Random(4101)
    a, b = bc.rand_seq(rnd, 200), bc.rand_seq(rnd, 5)
    qseq, src = bc.tile_records([a, b, "A" * 7], W, STEP, 1)
    assert src[0][2] == 3 and tc.starts(200, W, STEP) == [0, 64, 73]
    qseq[src[2][0] * W:src[2][0] * W + 7] = np.arange(25, 32)
    db = _db(rnd, 600)
    paths = [
        (0, 100, [200 << 4 | 0]),
        (3, 60, [1 << 4 | (0, 2, 3)[k % 3] for k in range(130)]),
        (0, 7, []),
        (0, 300, fc.runs("=X=I=")),
        (0, 40, fc.runs("=X=X=X=")),
        (64, 200, fc.runs("=" * 9 + "D" * 3 + "X" * 64 + "I" * 2 + "=")),   # from a tile start on
    ]
    rec, ops = _paths(paths)
    return RowSet(qseq, W, STEP, db, tx.blosum62(), [src[0], src[0], src[0], src[1], src[2], src[0]], rec, ops, 0)


def hand_frame_set(strand):
    """A read of six frames of 200 letters (strand 0 begins at frame 0 of the
    tile table, strand 1 at frame 3) and one of six frames of 5 letters. Paths:
    66 and more words with a '\\' as word 63 and a '/' as word 64 (a shift on
    each side of the word-group boundary); a '/' after a pair at strand position
    3c + 0, which steps to frame 2 of letter c (the signed advance); a '/' that
    lands on strand position 3 * 128, the first letter read from the last,
    flush-right tile, and a '\\' landing on 3 * 128 + 1; the empty path and the
    one-tile source."""
    import tbext_cases as tx

    rnd = random.Random(4201 + strand)
    big = [bc.rand_seq(rnd, 200) for _ in range(6)]
    small = [bc.rand_seq(rnd, 5) for _ in range(6)]
    qseq, src6 = bc.tile_records(big + small, W, STEP, 6)
    assert src6[3][0] == 3 and src6[0][2] == 3
    s_big, s_small = src6[3 * strand], src6[6 + 3 * strand]
    db = _db(rnd, 600)
    words = [1 << 4 | k % 2 for k in range(63)] + [1 << 4 | 4, 1 << 4 | 5] + fc.runs("=X==D=II=")
    assert len(words) >= 66 and words[63] & 15 == 4 and words[64] & 15 == 5
    paths = [
        (0, 50, words),
        (30, 300, fc.runs("=/===X\\==")),
        (370, 100, fc.runs("=====/" + "=" * 10)),
        (381 - 6, 120, fc.runs("=X=\\" + "=" * 70 + "I=")),
        (0, 9, []),
        (1, 400, fc.runs("==\\=/X")),
        (599 - 3 * 70, 200, fc.runs("=" * 71)),     # up to the strand's last position
    ]
    rec, ops = _paths(paths)
    src = [s_big, s_big, s_big, s_big, s_big, s_small, s_big]
    return RowSet(qseq, W, STEP, db, tx.blosum62(), src, rec, ops, 1, shift=-15)


def made_band_set(case):
    """The band pass's own paths of a band_cases stage case (host model)."""
    rec, ops = case.host()
    return RowSet(case.qseq, case.W, case.step, case.db, case.M(), case.src, rec, ops, 0, gaps=case.gaps)


def made_frame_set(case):
    """The frame pass's own paths of a frame_cases stage case (host model)."""
    rec, ops = case.host()
    return RowSet(case.qseq, case.W, case.step, case.db, case.M(), case.src, rec, ops, 1, gaps=case.gaps, shift=case.shift)


def stage_sets():
    """(id, builder) of the sets the device is checked on: the hand-made paths on
    both strand layouts, the planted truths and one mixed case each at B = 31."""
    return [
        ("hand_band", hand_band_set),
        ("hand_frame_strand0", lambda: hand_frame_set(0)),
        ("hand_frame_strand1", lambda: hand_frame_set(1)),
        ("truth_ins", lambda: made_frame_set(fc.truth_case(77, "ins")[0])),
        ("truth_del", lambda: made_frame_set(fc.truth_case(77, "del")[0])),
        ("band_mixed_B31", lambda: made_band_set(bc.mixed_case(5, 2 * W + STEP + 3, B=31, n=21))),
        ("frame_mixed_B31", lambda: made_frame_set(fc.mixed_case(9, 200, 31, n=13))),
    ]


# ---------------------------------------------------------------- stage level
_p = bc._p
stage_setup = bc.stage_setup


def gpu_rows(lib, rs, count=None, rows=True):
    """ReadRowsGpu on the resident chunks: the size first (rows == NULL), then the
    bytes into a buffer with guard bytes behind them. Returns (rec, rows)."""
    from ghostm_amd import READ_ROWS_DTYPE, native

    n = len(rs.src) if count is None else count
    src, rec = np.ascontiguousarray(rs.src[:n]), np.ascontiguousarray(rs.rec[:n])
    out = np.zeros(n + 1, dtype=READ_ROWS_DTYPE)
    out["columns"][n] = 0xDEADBEEF

    def call(outp, buf, cap, used):
        return lib.ReadRowsGpu(n, src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                               rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), _p(rs.ops), len(rs.ops), rs.W,
                               rs.step, rs.frame, rs.gaps[0], rs.gaps[1], rs.shift, outp, buf, cap, ctypes.byref(used))

    used = ctypes.c_size_t(12345)
    assert call(None, None, 0, used) == 0, native.last_error()
    need = used.value
    if not rows:
        assert call(out.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)), None, 0, used) == 0, native.last_error()
        return out[:n], None
    buf = np.full(need + 16, 0xA7, dtype=np.uint8)
    used2 = ctypes.c_size_t(12345)
    assert call(out.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)), _p(buf, ctypes.c_uint8), need, used2) == 0, \
        native.last_error()
    assert used2.value == need and (buf[need:] == 0xA7).all() and out["columns"][n] == 0xDEADBEEF
    return out[:n], buf[:need]


def refusal_variants(rs):
    """(reason, keyword arguments of a raw call) of every refusal the contract
    names, on a frame set whose hit 1 has words."""
    def src_with(**kw):
        s = rs.src.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s

    def rec_with(**kw):
        r = rs.rec.copy()
        for k, v in kw.items():
            r[k][1] = v
        return r

    def ops_with(word):
        o = rs.ops.copy()
        o[int(rs.rec["ops_offset"][1])] = word
        return o

    out = [
        ("source", dict(src=src_with(first_record=rs.nq))),
        ("source", dict(src=src_with(tiles=0))),
        ("source", dict(src=src_with(letters=0))),
        ("source", dict(src=src_with(tiles=int(rs.src["tiles"][1]) + 1))),
        ("source", dict(src=src_with(stride=0))),
        ("source", dict(step=0)),
        ("source", dict(step=rs.W + 1)),
        ("ops", dict(rec=rec_with(ops_offset=len(rs.ops)))),
        ("word", dict(ops=ops_with(0 << 4 | 0))),
        ("word", dict(ops=ops_with(1 << 4 | 8))),
        ("word", dict(ops=ops_with(1 << 4 | (6 if rs.frame else 4)))),
        ("bounds", dict(rec=rec_with(q_start=(3 if rs.frame else 1) * int(rs.src["letters"][1])))),
        ("bounds", dict(rec=rec_with(q_start=(3 if rs.frame else 1) * int(rs.src["letters"][1]) - 1))),
        ("bounds", dict(rec=rec_with(s_start=len(rs.db) - 2))),
        ("rows_cap", dict(rows_cap=5)),
        ("null", dict(null_src=True)),
    ]
    if rs.frame:
        out += [("word", dict(ops=ops_with(1 << 4 | 7))), ("shift", dict(shift=1)), ("shift", dict(shift=-(1 << 20) - 1)),
                ("bounds", dict(rec=rec_with(q_start=0), ops=ops_with(1 << 4 | 5))),   # a '/' first: below position 0
                ("source", dict(nq=int(rs.src["first_record"][1]) + 6 * (int(rs.src["tiles"][1]) - 1) + 2))]
    else:
        out += [("word", dict(ops=ops_with(1 << 4 | 5))),
                ("source", dict(nq=int(rs.src["first_record"][1]) + int(rs.src["tiles"][1]) - 1))]
    return out
