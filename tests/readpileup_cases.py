"""Shared by tests/test_read_pileup_host.py, tests/test_gpu_read_pileup.py and
tests/readpileup_poison_child.py (not a test module): a Python model of the
read-level subject pile-up written from its contract, the calls into guarded
outputs, the tile-edge path sets and the session-level model.

The contract (include/ghostm_hip.h, ReadPileupGpu). A profile row is 32
counters per position of the DB chunk; slot(c) = c below 25, else 25. A hit is a
source (first_record, stride, tiles, letters) and a path (q_start, s_start
absolute in the chunk, words length << 4 | op); its query letters are read
through the source as the read-level rows read them (readrows_cases.locate).
Band mode: a column of op 0 or 1 at subject position s adds 1 to row s, slot of
the letter at the position, and advances both by 1; op 2 advances the position
only; op 3 adds 1 to row s, slot 26, and advances the subject. Frame mode: the
position p is in nucleotides, a column of op 0, 1 or 2 reads letter p // 3 of
frame p % 3 and advances p by 3; a column of op 4 adds 1 to slot 27 of the row
the path stands at (s_start + the subject residues of the columns before it)
and advances p by 1; op 5 adds 1 to slot 28 there and takes 1 from p. Per
position: depth = the sum of slots 0..26, identities = the slot of the DB
residue, consensus = the largest of slots 0..24 (the lowest on a tie, 255 when
all are 0), shifts = slot 27 + slot 28."""
from __future__ import annotations

import ctypes

import numpy as np

import band_cases as bc
import readrows_cases as rc

GUARD32, GUARD8, PAD = 0xDEADBEEF, 0xA7, 8
EDGE_ENV = {"GHOSTM_PILEUP_TILE": "32", "GHOSTM_PILEUP_PART_HITS": "7"}
NAMES = ("depth", "identities", "consensus", "shifts", "profile")


# ---------------------------------------------------------------- Python model
def add_paths(prof, qseq, W, step, src, rec, ops, frame, s_shift=None):
    """Adds every hit's columns to prof, column by column; s_shift[h] is added to
    hit h's s_start (session level)."""
    for h in range(len(rec)):
        p, s = int(rec["q_start"][h]), int(rec["s_start"][h]) + (0 if s_shift is None else int(s_shift[h]))
        for w in bc.hit_words(rec, ops, h):
            op, n = int(w) & 15, int(w) >> 4
            for _ in range(n):
                if op < 2:
                    r, b = rc.locate(src[h], p % 3, p // 3, W, step) if frame else rc.locate(src[h], 0, p, W, step)
                    prof[s, min(int(qseq[r * W + b]), 25)] += 1
                    s += 1
                elif op == 3:
                    prof[s, 26] += 1
                    s += 1
                elif op == 4:
                    prof[s, 27] += 1
                elif op == 5:
                    prof[s, 28] += 1
                if op <= 2:
                    p += 3 if frame else 1
                elif op == 4:
                    p += 1
                elif op == 5:
                    p -= 1


def finish(prof, db):
    """(depth, identities, consensus, shifts) of a profile (n, 32) over residues db."""
    n = len(db)
    depth = prof[:, :27].sum(axis=1, dtype=np.uint64).astype(np.uint32)
    ident = prof[np.arange(n), np.minimum(np.asarray(db, dtype=np.int64), 25)].astype(np.uint32)
    head = prof[:, :25]
    cons = np.where(head.max(axis=1, initial=0) > 0, head.argmax(axis=1), 255).astype(np.uint8) if n else \
        np.zeros(0, dtype=np.uint8)
    return depth, ident, cons, (prof[:, 27] + prof[:, 28]).astype(np.uint32)


def model(rs, count=None):
    """(depth, identities, consensus, shifts, profile) of a RowSet's first count hits."""
    n = len(rs.src) if count is None else count
    prof = np.zeros((len(rs.db), 32), dtype=np.uint32)
    add_paths(prof, rs.qseq, rs.W, rs.step, rs.src[:n], rs.rec[:n], rs.ops, rs.frame)
    return (*finish(prof, rs.db), prof)


# ---------------------------------------------------------------- calls
_p = bc._p


def _srcp(a):
    from ghostm_amd import native
    return a.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource))


def _recp(a):
    from ghostm_amd import native
    return a.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath))


def _opt(a, t=ctypes.c_uint32):
    return None if a is None else _p(a, t)


def host_call(lib, rs):
    """call(src, rec, ops, ops_len, W, step, frame, db_len, depth, ident, cons, shifts, prof, nq=None) -> rc for
    GhostmReadPileupHost on the set's chunks (db_len only chooses the output sizes)."""
    def call(src, rec, ops, ops_len, W, step, frame, db_len, depth, ident, cons, shifts, prof, nq=None, null_src=False):
        return lib.GhostmReadPileupHost(
            _p(rs.qseq, ctypes.c_uint8), rs.nq if nq is None else nq, rs.W, _p(rs.db, ctypes.c_uint8), len(rs.db),
            len(src), None if null_src else _srcp(src), _recp(rec), _p(ops), ops_len, W, step, frame, _opt(depth),
            _opt(ident), _opt(cons, ctypes.c_uint8), _opt(shifts), _opt(prof))
    return call


def gpu_call(lib):
    """The same for ReadPileupGpu on the resident chunks (rc.stage_setup)."""
    def call(src, rec, ops, ops_len, W, step, frame, db_len, depth, ident, cons, shifts, prof, nq=None, null_src=False):
        return lib.ReadPileupGpu(len(src), None if null_src else _srcp(src), _recp(rec), _p(ops), ops_len, W, step, frame,
                                 db_len, _opt(depth), _opt(ident), _opt(cons, ctypes.c_uint8), _opt(shifts), _opt(prof))
    return call


def guarded(db_len, shifts=True, profile=True):
    return [np.full(db_len + PAD, GUARD32, dtype=np.uint32), np.full(db_len + PAD, GUARD32, dtype=np.uint32),
            np.full(db_len + PAD, GUARD8, dtype=np.uint8),
            np.full(db_len + PAD, GUARD32, dtype=np.uint32) if shifts else None,
            np.full((db_len + PAD) * 32, GUARD32, dtype=np.uint32) if profile else None]


def untouched(outs):
    return all(o is None or (o == (GUARD8 if o.dtype == np.uint8 else GUARD32)).all() for o in outs)


def pileup_via(call, rs, count=None, shifts=True, profile=True):
    """One call into guard-filled outputs; nothing is written behind db_len
    elements. Returns (depth, identities, consensus, shifts or None, profile or None)."""
    from ghostm_amd import native

    n = len(rs.src) if count is None else count
    src, rec = np.ascontiguousarray(rs.src[:n]), np.ascontiguousarray(rs.rec[:n])
    db_len = len(rs.db)
    outs = guarded(db_len, shifts, profile)
    assert call(src, rec, rs.ops, len(rs.ops), rs.W, rs.step, rs.frame, db_len, *outs) == 0, native.last_error()
    res = []
    for o, width in zip(outs, (1, 1, 1, 1, 32)):
        if o is None:
            res.append(None)
            continue
        assert (o[db_len * width:] == (GUARD8 if o.dtype == np.uint8 else GUARD32)).all()
        res.append(o[:db_len * width].reshape(db_len, 32) if width == 32 else o[:db_len])
    return tuple(res)


def assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            continue
        bad = np.nonzero(np.asarray(g) != np.asarray(w))
        assert len(bad[0]) == 0, (what, name, [b[:5].tolist() for b in bad])


def check_against_model(call, rs, what, count=None, want=None):
    """With and without the profile, with and without shifts, against the Python
    model. Returns the model's arrays."""
    want = model(rs, count) if want is None else want
    for shifts, profile in ((True, True), (False, False), (True, False), (False, True)):
        assert_same(pileup_via(call, rs, count, shifts, profile), want, (what, shifts, profile))
    prof = want[4]
    assert (prof[:, 29:] == 0).all() and np.array_equal(want[0], prof[:, :27].sum(axis=1))
    if not rs.frame:
        assert (prof[:, 27:] == 0).all()
    return want


# ---------------------------------------------------------------- the smallest shapes that can break
def _reads(seed, strand=0):
    """(qseq, band source, frame source of the strand) of a read of six frames of
    200 letters at W = 127, step 64: three tile records per frame."""
    import random
    rnd = random.Random(seed)
    qseq, src6 = bc.tile_records([bc.rand_seq(rnd, 200) for _ in range(6)], rc.W, rc.STEP, 6)
    assert src6[0][2] == 3
    return rnd, qseq, src6[3 * strand]


def _set(rnd, qseq, src, paths, frame, db=None):
    import tbext_cases as tx
    db = rc._db(rnd, 600) if db is None else db
    rec, ops = rc._paths(paths)
    return rc.RowSet(qseq, rc.W, rc.STEP, db, tx.blosum62(), [src] * len(paths), rec, ops, frame)


def edge_sets(strand=0, offset=0, residues=600):
    """name -> RowSet, for tiles of 32 positions and parts of 7 hits; the DB
    chunk has residues + 2 positions (an END, the residues, an END). offset moves
    every path that is not tied to an end of the chunk (a multiple of 32 keeps
    the tile edges where they are)."""
    w = lambda n, op: n << 4 | op  # noqa: E731
    E, X, I, D, UP, DOWN = 0, 1, 2, 3, 4, 5
    rnd, qseq, src = _reads(4401 + strand, strand)
    db = rc._db(rnd, residues)
    n = len(db)
    alt = [w(1, k % 2) for k in range(64)]
    frame = {
        # positions 30..179 (tiles 0 to 5); letters 0..149 change record at 64 and at 128, inside tiles 2 and 4
        "four_tiles": [(0, 30, [w(150, E)])],
        "d_across_edge": [(3, 50, [w(12, E), w(10, D), w(8, X)])],                   # D at 62..71
        # pairs at 60..63, the shift charged to 64, the first position of tile 2
        "up_at_tile_start": [(0, 60, [w(4, E), w(1, UP), w(3, X)])],
        "down_at_tile_start": [(30, 92, [w(4, E), w(1, DOWN), w(3, X)])],            # charged to 96
        # 63 words end at 128 = tile 4's first position, word 64 (the group's last) is the shift charged there
        "shift_ends_group": [(0, 65, alt[:63] + [w(1, UP), w(2, E)])],
        # 64 words end at 160, word 65 is a shift: a group of its own, one past the path's last residue
        "shift_after_group": [(6, 96, alt + [w(2, DOWN)])],
        "ends_in_shift": [(0, 20, [w(12, E), w(1, UP)])],                            # charged to 32, residues end at 31
        "ends_in_shift_at_chunk_end": [(0, n - 11, [w(10, X), w(1, UP)])],           # charged to the chunk's last position
        "position_1": [(2, 1, [w(1, UP), w(1, E)])],
        "last_residue": [(9, n - 41, [w(20, X), w(1, DOWN), w(10, D), w(10, E)])],          # ends on residue 600
        "i_at_edge": [(5, 54, [w(10, E), w(5, I), w(1, UP), w(10, E)])],             # shift at 64 after an insertion
        "copies_300": [(60, 70, [w(9, E), w(1, UP), w(11, X)])] * 300,
    }
    fixed = ("position_1", "last_residue", "ends_in_shift_at_chunk_end")
    move = lambda sets: {k: [(q, s0 if k in fixed else s0 + offset, ws) for q, s0, ws in v] for k, v in sets.items()}  # noqa: E731
    frame = move(frame)
    mixed = [p[0] for k, p in frame.items() if k != "copies_300"] + [(0, 9, [])]
    frame["mixed"] = mixed
    frame["mixed_reversed"] = mixed[::-1]
    out = {"frame_" + k: _set(rnd, qseq, src, v, 1, db) for k, v in frame.items()}
    band = {
        "four_tiles": [(0, 30, [w(150, E)])],
        "d_across_edge": [(3, 50, [w(12, E), w(10, D), w(8, X)])],
        "position_1": [(2, 1, [w(1, E)])],
        "last_residue": [(9, n - 51, [w(20, X), w(10, D), w(20, E)])],
        "i_at_edge": [(5, 54, [w(10, E), w(5, I), w(10, E)])],
        "copies_300": [(60, 70, [w(20, E)])] * 300,
    }
    band = move(band)
    mixed = [p[0] for k, p in band.items() if k != "copies_300"] + [(0, 9, [])]
    band["mixed"] = mixed
    band["mixed_reversed"] = mixed[::-1]
    out.update({"band_" + k: _set(rnd, qseq, src, v, 0, db) for k, v in band.items()})
    return out


def expected_edges(name, want):
    """What the edge sets must show whatever the implementation."""
    depth, shifts, prof = want[0], want[3], want[4]
    if name == "frame_up_at_tile_start":
        assert np.flatnonzero(shifts).tolist() == [64] and prof[64, 27] == 1 and depth[60:67].tolist() == [1] * 7
    if name == "frame_down_at_tile_start":
        assert np.flatnonzero(shifts).tolist() == [96] and prof[96, 28] == 1
    if name == "frame_shift_ends_group":
        assert np.flatnonzero(shifts).tolist() == [128] and int(depth.sum()) == 65
    if name == "frame_shift_after_group":
        assert shifts[160] == 2 and depth[160] == 0 and depth[159] == 1 and int(shifts.sum()) == 2
    if name == "frame_ends_in_shift":
        assert shifts[32] == 1 and depth[32] == 0 and int(depth.sum()) == 12
    if name == "frame_ends_in_shift_at_chunk_end":
        assert shifts[-1] == 1 and int(shifts.sum()) == 1
    if name.endswith("copies_300"):
        assert int(depth.max()) == 300 and int(prof.max()) == 300
    if name == "frame_copies_300":
        assert shifts[79] == 300
    if name.endswith("d_across_edge"):
        assert prof[62:72, 26].tolist() == [1] * 10


# ---------------------------------------------------------------- refusals
def refusal_cases(rs):
    """(reason, keyword arguments) of every refused call: the read-level rows'
    own (readrows_cases.refusal_variants, without those of arguments this call
    does not take) and the pile-up's."""
    out = [(r, kw) for r, kw in rc.refusal_variants(rs) if r not in ("rows_cap", "shift")]
    out.append(("null", dict(null_depth=True)))
    if rs.frame:  # a shift column standing at db_len, behind a path that ends on the chunk's last position
        rec = rs.rec.copy()
        ops = np.concatenate([rs.ops, np.array([3 << 4 | 0, 1 << 4 | 4], dtype=np.uint32)])
        rec["q_start"][1], rec["s_start"][1], rec["n_runs"][1], rec["ops_offset"][1] = 0, len(rs.db) - 3, 2, len(rs.ops)
        out.append(("bounds", dict(rec=rec, ops=ops)))
    return out


def check_refusals(call, rs, gpu):
    """Every refusal names its reason and leaves guard-filled outputs as they were."""
    from ghostm_amd import native

    db_len = len(rs.db)
    todo = [(r, kw) for r, kw in refusal_cases(rs) if not (gpu and "nq" in kw)]
    if gpu:
        todo += [("db_len", dict(db_len=db_len - 1)), ("db_len", dict(db_len=db_len + 1)), ("source", dict(W=rs.W - 1))]
    seen = set()
    for reason, kw in todo:
        src = np.ascontiguousarray(kw.get("src", rs.src))
        rec = np.ascontiguousarray(kw.get("rec", rs.rec))
        ops = np.ascontiguousarray(kw.get("ops", rs.ops))
        outs = guarded(db_len + 1)
        code = call(src, rec, ops, len(ops), kw.get("W", rs.W), kw.get("step", rs.step), rs.frame,
                    kw.get("db_len", db_len), None if kw.get("null_depth") else outs[0], *outs[1:], nq=kw.get("nq"),
                    null_src=bool(kw.get("null_src")))
        assert code != 0 and reason in native.last_error(), (reason, kw, native.last_error())
        assert untouched(outs), (reason, kw)
        seen.add(reason)
    assert seen == {"source", "ops", "word", "bounds", "null"} | ({"db_len"} if gpu else set())


# ---------------------------------------------------------------- stage sets
def stage_sets():
    """(id, builder) of the sets the device is checked on: readrows_cases' sets."""
    return rc.stage_sets()


# ---------------------------------------------------------------- session level
def session_model(s, W, step, frame, path, ops, dna=True):
    """The Python model applied to a session's read-level paths (hits_band() or
    hits_frame()), with the sources rebuilt from what the session shows
    (band_cases.session_inputs). Returns (subjects[READ_PILEUP_DTYPE], depth,
    identities, consensus, shifts, profile) over the concatenated subjects."""
    from ghostm_amd import BAND_SOURCE_DTYPE, READ_PILEUP_DTYPE

    inp = bc.session_inputs(s, W, step, dna=dna)
    hits = s.hits()
    tiles, qrec = s.query_tiles(), s.hits_rows()[0]["query_record"]
    per_hit = inp["per_hit"]
    profs = [np.zeros((len(d[3]), 32), dtype=np.uint32) for d in inp["dbs"]]
    groups = {}
    for h, x in enumerate(per_hit):
        groups.setdefault((x[0], x[1]), []).append(h)
    for (qi, di), idx in groups.items():
        back = [int(tiles["frame"][qrec[h]]) % 3 if frame else 0 for h in idx]
        src = np.array([(per_hit[h][2][0] - b,) + tuple(per_hit[h][2][1:]) for h, b in zip(idx, back)],
                       dtype=BAND_SOURCE_DTYPE)
        add_paths(profs[di], inp["chunks"][qi][2], W, step or W, src, path[idx], ops, frame,
                  s_shift=[per_hit[h][4] for h in idx])
    layout = []   # per subject in db_id order: (chunk, first position, length)
    for di, (dbase, starts, lens, codes) in enumerate(inp["dbs"]):
        layout += [(di, int(a), int(n)) for a, n in zip(starts, lens)]
    cut = lambda arrs: np.concatenate([arrs[di][a:a + n] for di, a, n in layout])  # noqa: E731
    prof = cut(profs)
    depth, ident, cons, shifts = finish(prof, cut([d[3] for d in inp["dbs"]]))
    subj = np.zeros(len(layout), dtype=READ_PILEUP_DTYPE)
    nhits = np.bincount(hits["db_id"], minlength=len(layout))
    at = 0
    for i, (di, a, n) in enumerate(layout):
        d = depth[at:at + n]
        subj[i] = (n, nhits[i], int((d > 0).sum()), int(d.max(initial=0)), int(d.sum(dtype=np.uint64)),
                   int(ident[at:at + n].sum(dtype=np.uint64)), at, int(shifts[at:at + n].sum(dtype=np.uint64)))
        at += n
    return subj, depth, ident, cons, shifts, prof


def charged_columns(path, ops):
    """(the '=', 'X' and 'D' columns, the shift columns) of a set of paths, from the words."""
    cols = shifts = 0
    for h in range(len(path)):
        for w in bc.hit_words(path, ops, h):
            op, n = int(w) & 15, int(w) >> 4
            cols += n if op in (0, 1, 3) else 0
            shifts += n if op >= 4 else 0
    return cols, shifts
