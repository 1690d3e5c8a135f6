"""Python face of the native `aln` engine, mirroring the reference C++ API.

    Aligner().execute(["aln", "-i", q, "-d", db, "-o", out, ...])
        reference Aligner::Execute (aligner.cpp:65-223) — same flags, same output.

    Session(argv)            inputs loaded once and resident in HBM; .run() is the
                             hot path (seed -> score -> merge -> traceback ->
                             E-value text), repeatable, with .output(), .hits(),
                             .stats().

    Session.for_queries(argv)  no database yet (-i optional); .set_db(seqs, names)
                             or .set_db_fasta(path) replace the database on the
                             live session (coded and indexed on the GPU): one
                             read set, many databases, no formatted files.

    Session.for_db(argv)     only the database resident; .set_queries(seqs, names)
                             or .set_queries_fasta(path) replace the query set on
                             the live session (coded and translated on the GPU),
                             then .run() as above: many read sets, one database.

Everything runs in libghostm_hip.so (HIP kernels for gfx950 + host merge); this
module only marshals arguments.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Sequence

import numpy as np

from . import native

HIT_DTYPE = np.dtype(
    [
        ("query_id", "<u4"),
        ("db_id", "<u4"),
        ("score", "<u4"),
        ("db_start", "<u4"),
        ("db_end", "<u4"),
        ("aln_len", "<u4"),
        ("aln_match", "<u4"),
        ("seq_id", "<f4"),
    ]
)

# GhostmHitExt: one per hit of Session.hits(), zero-based query coordinates
HIT_EXT_DTYPE = np.dtype([("q_start", "<u4"), ("q_end", "<u4"), ("mismatches", "<u4"), ("gap_opens", "<u4")])

# GhostmHitPath: one per hit, zero-based inclusive coordinates; the hit's
# run-length words are ops[ops_offset : ops_offset + n_runs]
HIT_PATH_DTYPE = np.dtype([("q_start", "<u4"), ("q_end", "<u4"), ("s_start", "<u4"), ("s_end", "<u4"),
                           ("score", "<u4"), ("n_runs", "<u4"), ("ops_offset", "<u8")])

PATH_OPS = "=XID"  # op codes 0..3 of a run-length word (length << 4 | op)


def cigar(ops) -> str:
    """The extended CIGAR of one hit's run-length words, for instance 31=1X2D40=."""
    return "".join(f"{int(w) >> 4}{PATH_OPS[int(w) & 3]}" for w in ops)


# GhostmHitRows: one per hit; the hit's 3 * columns bytes (query row, midline,
# subject row) are rows[rows_offset : rows_offset + 3 * columns]
HIT_ROWS_DTYPE = np.dtype([("query_record", "<u4"), ("columns", "<u4"), ("identities", "<u4"), ("positives", "<u4"),
                           ("gap_residues", "<u4"), ("rescore", "<i4"), ("rows_offset", "<u8")])


# GhostmQueryTile: one per output record of a tiled query set
QUERY_TILE_DTYPE = np.dtype([("record", "<u4"), ("offset", "<u4"), ("letters", "<u4"), ("frame", "<u4")])


def tile_plan(lengths, width: int = 75, dna: bool = False, max_len: int = 0, step: int = 1):
    """The tile table a tiled set_queries would make of records of these letter
    counts (GhostmQueryTilePlan; no device): (tiles[QUERY_TILE_DTYPE],
    cut_records). width, dna, max_len and step as given to set_queries."""
    lib = native.load()
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    cut = ctypes.c_uint64(0)
    args = (lens.ctypes.data_as(u32p), len(lens), int(width), int(bool(dna)), int(max_len), int(step))
    n = lib.GhostmQueryTilePlan(*args, None, 0, ctypes.byref(cut))
    if n < 0:
        raise GhostmError(native.last_error())
    out = np.zeros(n, dtype=QUERY_TILE_DTYPE)
    if n:
        lib.GhostmQueryTilePlan(*args, out.ctypes.data_as(ctypes.POINTER(native.GhostmQueryTile)), n, ctypes.byref(cut))
    return out, int(cut.value)


def rows_of(rec, rows, h) -> tuple[bytes, bytes, bytes]:
    """(query row, midline, subject row) of hit h of a (rec, rows) pair."""
    o, n = int(rec["rows_offset"][h]), int(rec["columns"][h])
    b = bytes(rows[o:o + 3 * n])
    return b[:n], b[n:2 * n], b[2 * n:]


# GhostmSubjectPileup: one per subject in db_id order; the subject's positions
# are [offset, offset + length) of the session-level pile-up arrays
SUBJECT_PILEUP_DTYPE = np.dtype([("length", "<u4"), ("hits", "<u4"), ("covered", "<u4"), ("max_depth", "<u4"),
                                 ("depth_sum", "<u8"), ("identities_sum", "<u8"), ("offset", "<u8")])

RESIDUE_LETTERS = b"ARNDCQEGHILKMFPSTWYVBJZX*"


def consensus_text(consensus, depth) -> bytes:
    """The pile-up's consensus as text: the residue letter, '-' where depth > 0
    and consensus is 255 (only codes from 25 up or deletions were seen), '.'
    where depth is 0."""
    c = np.asarray(consensus, dtype=np.uint8)
    d = np.asarray(depth)
    table = np.full(256, ord("-"), dtype=np.uint8)
    table[:25] = np.frombuffer(RESIDUE_LETTERS, dtype=np.uint8)
    out = table[c]
    out[d == 0] = ord(".")
    return out.tobytes()


class GhostmError(RuntimeError):
    pass


def traceback_ext_host(query_seqs, L, db, score_matrix, query_ids, db_ends, base_search_length,
                       open_gap=-11, extend_gap=-1):
    """The host model of the extended traceback (GhostmTraceBackExtHost; no
    device): query_seqs = uint8 codes of nq records of L, db = the END-separated
    uint8 codes of a DB chunk, score_matrix = 32x32 int32 M[db*32 + query].
    Returns (db_starts, aln_lens, aln_matches, ext[HIT_EXT_DTYPE])."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    qid = np.ascontiguousarray(query_ids, dtype=np.uint32)
    end = np.ascontiguousarray(db_ends, dtype=np.uint32)
    if m.size != 32 * 32 or L <= 0 or qs.size % L or qid.shape != end.shape:
        raise ValueError("traceback_ext_host: bad argument shapes")
    n = len(qid)
    start, alen, match = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    ext = np.zeros(n, dtype=HIT_EXT_DTYPE)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    rc = lib.GhostmTraceBackExtHost(
        qs.ctypes.data_as(u8p), qs.size // L, L, dbs.ctypes.data_as(u8p), dbs.size,
        m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n, qid.ctypes.data_as(u32p), end.ctypes.data_as(u32p),
        base_search_length, open_gap, extend_gap, start.ctypes.data_as(u32p), alen.ctypes.data_as(u32p),
        match.ctypes.data_as(u32p), ext.ctypes.data_as(ctypes.POINTER(native.GhostmHitExt)))
    if rc != 0:
        raise GhostmError(native.last_error())
    return start, alen, match, ext


def traceback_path_host(query_seqs, L, db, score_matrix, query_ids, db_ends, base_search_length,
                        open_gap=-11, extend_gap=-1, db_starts_in=None):
    """The host model of the path traceback (GhostmTraceBackPathHost; no device);
    arguments as traceback_ext_host, db_starts_in = the hits' known starts or
    None. Returns (records[HIT_PATH_DTYPE], ops[uint32])."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    qid = np.ascontiguousarray(query_ids, dtype=np.uint32)
    end = np.ascontiguousarray(db_ends, dtype=np.uint32)
    start = None if db_starts_in is None else np.ascontiguousarray(db_starts_in, dtype=np.uint32)
    if m.size != 32 * 32 or L <= 0 or qs.size % L or qid.shape != end.shape or (
            start is not None and start.shape != end.shape):
        raise ValueError("traceback_path_host: bad argument shapes")
    n = len(qid)
    rec = np.zeros(n, dtype=HIT_PATH_DTYPE)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)

    def call(ops, cap, used):
        rc = lib.GhostmTraceBackPathHost(
            qs.ctypes.data_as(u8p), qs.size // L, L, dbs.ctypes.data_as(u8p), dbs.size,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n, qid.ctypes.data_as(u32p), end.ctypes.data_as(u32p),
            None if start is None else start.ctypes.data_as(u32p), base_search_length, open_gap, extend_gap,
            rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), ops, cap, ctypes.byref(used))
        if rc != 0:
            raise GhostmError(native.last_error())

    used = ctypes.c_size_t(0)
    call(None, 0, used)  # the size needed
    ops = np.zeros(used.value, dtype=np.uint32)
    if used.value:
        call(ops.ctypes.data_as(u32p), used.value, used)
    return rec, ops


# GhostmBandSource: one source of the read-level band pass (its tile records in
# the query chunk, its letters)
BAND_SOURCE_DTYPE = np.dtype([("first_record", "<u4"), ("stride", "<u4"), ("tiles", "<u4"), ("letters", "<u4")])


def _band_call(fn, head, src, diagonal, s_lo, s_hi, W, step, band, open_gap, extend_gap, *more):
    """The band and frame entry points take the same tail: the size call, then
    the words. more: what follows extend_gap (the frame pass's shift cost)."""
    srcs = np.ascontiguousarray(src, dtype=BAND_SOURCE_DTYPE)
    diag = np.ascontiguousarray(diagonal, dtype=np.int32)
    lo = np.ascontiguousarray(s_lo, dtype=np.uint32)
    hi = np.ascontiguousarray(s_hi, dtype=np.uint32)
    if not (srcs.shape == diag.shape == lo.shape == hi.shape):
        raise ValueError("band align: bad argument shapes")
    n = len(srcs)
    rec = np.zeros(n, dtype=HIT_PATH_DTYPE)
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def call(ops, cap, used):
        rc = fn(*head, n, srcs.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                diag.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), lo.ctypes.data_as(u32p), hi.ctypes.data_as(u32p),
                int(W), int(step), int(band), int(open_gap), int(extend_gap), *more,
                rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), ops, cap, ctypes.byref(used))
        if rc != 0:
            raise GhostmError(native.last_error())

    used = ctypes.c_size_t(0)
    call(None, 0, used)  # the size needed
    ops = np.zeros(used.value, dtype=np.uint32)
    if used.value:
        call(ops.ctypes.data_as(u32p), used.value, used)
    return rec, ops


def band_align_host(query_seqs, W, db, score_matrix, src, diagonal, s_lo, s_hi, step, band=31,
                    open_gap=-11, extend_gap=-1):
    """The host model of the read-level band pass (GhostmBandAlignHost; no
    device): query_seqs = uint8 codes of nq tile records of W, db = the uint8
    codes of a DB chunk, score_matrix = 32x32 int32 M[db*32 + query], src =
    BAND_SOURCE_DTYPE records, diagonal / s_lo / s_hi per hit. Returns
    (records[HIT_PATH_DTYPE], ops[uint32])."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    if m.size != 32 * 32 or W <= 0 or qs.size % W:
        raise ValueError("band_align_host: bad argument shapes")
    u8p = ctypes.POINTER(ctypes.c_uint8)
    head = (qs.ctypes.data_as(u8p), qs.size // W, int(W), dbs.ctypes.data_as(u8p), dbs.size,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return _band_call(lib.GhostmBandAlignHost, head, src, diagonal, s_lo, s_hi, W, step, band, open_gap, extend_gap)


def band_align_gpu(src, diagonal, s_lo, s_hi, W, step, band=31, open_gap=-11, extend_gap=-1):
    """BandAlignGpu on the chunks of SetQueryGpu / SetDbGpu; arguments and
    result as band_align_host."""
    lib = native.load()
    return _band_call(lib.BandAlignGpu, (), src, diagonal, s_lo, s_hi, W, step, band, open_gap, extend_gap)


def stage_band_stats() -> dict:
    """The band counters behind the stage-level calls (GhostmStageBandStats)."""
    lib = native.load()
    st = native.GhostmBandStats()
    lib.GhostmStageBandStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


def _mask_call(fn, query_seqs, W, src, step, window, trigger, extend):
    qs = np.array(query_seqs, dtype=np.uint8).reshape(-1)  # a copy: the call masks in place
    if W <= 0 or qs.size % W:
        raise ValueError("mask records: bad argument shapes")
    srcs = np.ascontiguousarray(src, dtype=BAND_SOURCE_DTYPE).reshape(-1)
    nq = qs.size // W
    masked = np.zeros(nq, dtype=np.uint32)
    args = [int(v) for v in (step, window, trigger, extend)]
    if any(not 0 <= v < 1 << 32 for v in args):
        raise GhostmError("mask records: an argument beyond 32 bits")
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    rc = fn(qs.ctypes.data_as(u8p), nq, int(W), len(srcs), srcs.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
            *args, masked.ctypes.data_as(u32p))
    if rc != 0:
        raise GhostmError(native.last_error())
    return qs, masked


def mask_records_host(query_seqs, W, src, step, window=12, trigger=220, extend=250):
    """The host model of the low-complexity mask (GhostmMaskRecordsHost; no
    device): query_seqs = uint8 codes of nq records of W, src =
    BAND_SOURCE_DTYPE records (sources that share no record), step = the tile
    step. Returns (records, masked): a masked copy of the records (masked
    letters are code 23) and the letters masked in every record. Raises
    GhostmError with the reason ("window", "levels", "source", "overlap")."""
    return _mask_call(native.load().GhostmMaskRecordsHost, query_seqs, W, src, step, window, trigger, extend)


def mask_records(query_seqs, W, src, step, window=12, trigger=220, extend=250):
    """MaskRecordsGpu: the same through the kernels, on a chunk of its own;
    arguments, result and refusals as mask_records_host (W at most 127)."""
    return _mask_call(native.load().MaskRecordsGpu, query_seqs, W, src, step, window, trigger, extend)


def stage_mask_stats() -> dict:
    """The mask counters behind the stage-level call (GhostmStageMaskStats)."""
    lib = native.load()
    st = native.GhostmMaskStats()
    lib.GhostmStageMaskStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmQualOut: one read's record of the quality stage
QUAL_OUT_DTYPE = np.dtype([("begin", "<u4"), ("kept", "<u4"), ("masked", "<u4"), ("bad", "<u4")])


def _qual_call(fn, letters, quals, offsets, lengths, trim, mask, min_len):
    ls = np.array(np.frombuffer(bytes(letters), dtype=np.uint8))  # a copy: the call masks in place
    qs = np.frombuffer(bytes(quals), dtype=np.uint8)
    if ls.size != qs.size:
        raise ValueError("quality trim: letters and qualities differ in size")
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    lens = np.ascontiguousarray(lengths, dtype=np.uint32).reshape(-1)
    if offs.size != lens.size:
        raise ValueError("quality trim: one offset per length")
    args = [int(v) for v in (trim, mask, min_len)]
    if any(not 0 <= v < 1 << 32 for v in args):
        raise GhostmError("quality trim: param: an argument beyond 32 bits")
    out = np.zeros(lens.size, dtype=QUAL_OUT_DTYPE)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lp = ls.ctypes.data_as(u8p) if ls.size else None
    qp = qs.ctypes.data_as(u8p) if qs.size else None
    rc = fn(lp, qp, int(ls.size), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), lens.ctypes.data_as(_U32P),
            int(lens.size), *args, out.ctypes.data_as(ctypes.POINTER(native.GhostmQualOut)))
    if rc != 0:
        raise GhostmError(native.last_error())
    return ls.tobytes(), out


def quality_trim_host(letters, quals, offsets, lengths, trim=20, mask=0, min_len=0):
    """The host model of the quality stage (GhostmQualityTrimHost; no device):
    read r is lengths[r] bytes at offsets[r] of letters and of quals (bytes,
    Phred+33). Returns (letters, out): a copy of the letters with the masked
    ones stored as N, and one QUAL_OUT_DTYPE record per read. Raises
    GhostmError with the reason ("param", "null", "record", "length")."""
    return _qual_call(native.load().GhostmQualityTrimHost, letters, quals, offsets, lengths, trim, mask, min_len)


def quality_trim(letters, quals, offsets, lengths, trim=20, mask=0, min_len=0):
    """QualityTrimGpu: the same through k_qual_trim; arguments, result and
    refusals as quality_trim_host."""
    return _qual_call(native.load().QualityTrimGpu, letters, quals, offsets, lengths, trim, mask, min_len)


def stage_qual_stats() -> dict:
    """The quality counters behind the stage-level call (GhostmStageQualStats)."""
    lib = native.load()
    st = native.GhostmQualStats()
    lib.GhostmStageQualStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmAdapterOut: one read's record of the adapter stage
ADAPTER_OUT_DTYPE = np.dtype([("kept", "<u4"), ("adapter_at", "<u4"), ("pair_len", "<u4"),
                              ("adapter_mismatches", "<u2"), ("pair_mismatches", "<u2")])


def _adapter_text(adapter) -> bytes:
    text = adapter.encode("latin-1") if isinstance(adapter, str) else bytes(adapter)
    if b"\0" in text:
        raise GhostmError("adapter trim: adapter: a NUL byte")
    return text


def _adapter_call(fn, letters, offsets, lengths, adapter1, adapter2, min_overlap, err_pct, pair_overlap):
    ls = np.frombuffer(letters, dtype=np.uint8)  # no copy: the call only reads them
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    lens = np.ascontiguousarray(lengths, dtype=np.uint32).reshape(-1)
    if offs.size != lens.size:
        raise ValueError("adapter trim: one offset per length")
    args = [int(v) for v in (min_overlap, err_pct, pair_overlap)]
    if any(not 0 <= v < 1 << 32 for v in args):
        raise GhostmError("adapter trim: param: an argument beyond 32 bits")
    out = np.zeros(lens.size, dtype=ADAPTER_OUT_DTYPE)
    lp = ls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if ls.size else None
    rc = fn(lp, int(ls.size), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), lens.ctypes.data_as(_U32P),
            int(lens.size), _adapter_text(adapter1), _adapter_text(adapter2), *args,
            out.ctypes.data_as(ctypes.POINTER(native.GhostmAdapterOut)))
    if rc != 0:
        raise GhostmError(native.last_error())
    return out


def adapter_trim_host(letters, offsets, lengths, adapter1="", adapter2="", min_overlap=5, err_pct=10, pair_overlap=0):
    """The host model of the adapter stage (GhostmAdapterTrimHost; no device):
    read r is lengths[r] bytes at offsets[r] of letters; adapter1 is looked for
    at every read's 3' end (adapter2, when given, in the odd records), and with
    pair_overlap > 0 records 2i and 2i + 1 are mates whose read-through is found
    from their overlap. Returns one ADAPTER_OUT_DTYPE record per read; the
    letters are not changed. Raises GhostmError with the reason ("param",
    "adapter", "null", "record", "length", "pairs")."""
    return _adapter_call(native.load().GhostmAdapterTrimHost, letters, offsets, lengths, adapter1, adapter2,
                         min_overlap, err_pct, pair_overlap)


def adapter_trim(letters, offsets, lengths, adapter1="", adapter2="", min_overlap=5, err_pct=10, pair_overlap=0):
    """AdapterTrimGpu: the same through k_adapter_find and k_pair_overlap;
    arguments, result and refusals as adapter_trim_host."""
    return _adapter_call(native.load().AdapterTrimGpu, letters, offsets, lengths, adapter1, adapter2, min_overlap,
                         err_pct, pair_overlap)


def stage_adapter_stats() -> dict:
    """The adapter counters behind the stage-level call (GhostmStageAdapterStats)."""
    lib = native.load()
    st = native.GhostmAdapterStats()
    lib.GhostmStageAdapterStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmHitFrameInfo: one per hit beside Session.hits_frame()'s records
HIT_FRAME_INFO_DTYPE = np.dtype([("strand", "<u4"), ("read_nt", "<u4"), ("letters", "<u4"), ("shifts", "<u4")])
# the operations of a frame path's words: PATH_OPS and the two shifts
FRAME_OPS = "=XID\\/"


def frame_cigar(ops) -> str:
    """The CIGAR of one hit's frame-path words as -y 13 prints it, for instance
    30=1\\29= ('\\': the next codon starts one nucleotide late, '/': early)."""
    return "".join(f"{int(w) >> 4}{FRAME_OPS[int(w) & 7]}" for w in ops)


def frame_align_host(query_seqs, W, db, score_matrix, src, diagonal, s_lo, s_hi, step, band=31,
                     open_gap=-11, extend_gap=-1, shift_cost=-15):
    """The host model of the frameshift-aware read-level pass
    (GhostmFrameAlignHost; no device). Arguments as band_align_host, with src
    naming frame 0 of each hit's strand (its frames g in records first_record +
    g + stride * t), and the frameshift cost. Returns (records[HIT_PATH_DTYPE]
    in strand positions, ops[uint32] with the op codes 0..5)."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    if m.size != 32 * 32 or W <= 0 or qs.size % W:
        raise ValueError("frame_align_host: bad argument shapes")
    u8p = ctypes.POINTER(ctypes.c_uint8)
    head = (qs.ctypes.data_as(u8p), qs.size // W, int(W), dbs.ctypes.data_as(u8p), dbs.size,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return _band_call(lib.GhostmFrameAlignHost, head, src, diagonal, s_lo, s_hi, W, step, band, open_gap, extend_gap,
                      int(shift_cost))


def frame_align(src, diagonal, s_lo, s_hi, W, step, band=31, open_gap=-11, extend_gap=-1, shift_cost=-15):
    """FrameAlignGpu on the chunks of SetQueryGpu / SetDbGpu; arguments and
    result as frame_align_host."""
    lib = native.load()
    return _band_call(lib.FrameAlignGpu, (), src, diagonal, s_lo, s_hi, W, step, band, open_gap, extend_gap,
                      int(shift_cost))


def stage_frame_stats() -> dict:
    """The frame counters behind the stage-level calls (GhostmStageFrameStats)."""
    lib = native.load()
    st = native.GhostmFrameStats()
    lib.GhostmStageFrameStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmHitReadRows: the rows record of a read-level path; HIT_ROWS_DTYPE's
# fields, then the shift columns
READ_ROWS_DTYPE = np.dtype(HIT_ROWS_DTYPE.descr + [("shifts", "<u4"), ("pad", "<u4")])


def _read_rows_call(fn, head, src, rec, ops, W, step, frame, open_gap, extend_gap, shift_cost):
    """ReadRowsGpu and GhostmReadRowsHost take the same tail: the size call,
    then the rows."""
    srcs = np.ascontiguousarray(src, dtype=BAND_SOURCE_DTYPE)
    p = np.ascontiguousarray(rec, dtype=HIT_PATH_DTYPE)
    w = np.ascontiguousarray(ops, dtype=np.uint32)
    if srcs.shape != p.shape:
        raise ValueError("read rows: bad argument shapes")
    n = len(srcs)
    out = np.zeros(n, dtype=READ_ROWS_DTYPE)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)

    def call(rows, cap, used):
        rc = fn(*head, n, srcs.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                p.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), w.ctypes.data_as(u32p), w.size, int(W),
                int(step), int(bool(frame)), int(open_gap), int(extend_gap), int(shift_cost),
                out.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)), rows, cap, ctypes.byref(used))
        if rc != 0:
            raise GhostmError(native.last_error())

    used = ctypes.c_size_t(0)
    call(None, 0, used)  # the size needed
    rows = np.zeros(used.value, dtype=np.uint8)
    if used.value:
        call(rows.ctypes.data_as(u8p), used.value, used)
    return out, rows


def read_rows_host(query_seqs, W, db, score_matrix, src, rec, ops, step, frame=False, open_gap=-11, extend_gap=-1,
                   shift_cost=-15):
    """The host model of the read-level rows (GhostmReadRowsHost; no device):
    query_seqs = the chunk's records of W codes, db = the chunk's residues, src
    = BAND_SOURCE_DTYPE records, rec = HIT_PATH_DTYPE records of band paths
    (frame False) or frame paths (frame True) with s_start absolute in the
    chunk, ops = the words they index. Returns (records[READ_ROWS_DTYPE],
    rows[uint8]); rows_of(rec, rows, h) is hit h's three rows."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    if m.size != 32 * 32 or W <= 0 or qs.size % W:
        raise ValueError("read_rows_host: bad argument shapes")
    u8p = ctypes.POINTER(ctypes.c_uint8)
    head = (qs.ctypes.data_as(u8p), qs.size // W, int(W), dbs.ctypes.data_as(u8p), dbs.size,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return _read_rows_call(lib.GhostmReadRowsHost, head, src, rec, ops, W, step, frame, open_gap, extend_gap,
                           shift_cost)


def read_rows(src, rec, ops, W, step, frame=False, open_gap=-11, extend_gap=-1, shift_cost=-15):
    """ReadRowsGpu on the chunks of SetQueryGpu / SetDbGpu; arguments and
    result as read_rows_host."""
    lib = native.load()
    return _read_rows_call(lib.ReadRowsGpu, (), src, rec, ops, W, step, frame, open_gap, extend_gap, shift_cost)


def stage_read_rows_stats() -> dict:
    """The read-rows counters behind the stage-level calls (GhostmStageReadRowsStats)."""
    lib = native.load()
    st = native.GhostmReadRowsStats()
    lib.GhostmStageReadRowsStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


def query_chunk_cuts(lengths, chunk_mb: int = 0, dna: bool = False) -> np.ndarray:
    """`ghostm qry`'s chunk cuts over records of these letter counts
    (GhostmQueryChunkCuts; no device): chunk c is records [cuts[c], cuts[c + 1]).
    chunk_mb and dna as qry's -L (0: the default) and -t d."""
    lib = native.load()
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    cuts = np.zeros(len(lens) + 1, dtype=np.uint64)
    n = lib.GhostmQueryChunkCuts(lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(lens), int(chunk_mb),
                                 int(bool(dna)), cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(cuts))
    if n < 0:
        raise GhostmError(native.last_error())
    return cuts[: n + 1]


def db_chunk_cuts(lengths, chunk_mb: int = 0) -> np.ndarray:
    """`ghostm db`'s chunk cuts over records of these letter counts
    (GhostmDbChunkCuts; no device): chunk c is records [cuts[c], cuts[c + 1]).
    chunk_mb as db's -l (0: the default). Raises when a record alone is over
    the limit, the first one included, and when chunk_mb is above 2047."""
    lib = native.load()
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    cuts = np.zeros(len(lens) + 1, dtype=np.uint64)
    n = lib.GhostmDbChunkCuts(lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(lens), int(chunk_mb),
                              cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(cuts))
    if n < 0:
        raise GhostmError(native.last_error())
    return cuts[: n + 1]


def path_rows_host(query_seqs, L, db, score_matrix, query_ids, rec, ops, open_gap=-11, extend_gap=-1):
    """The host model of the aligned rows (GhostmPathRowsHost; no device):
    query_seqs = the chunk's records of L codes, db = the chunk's residues, rec =
    HIT_PATH_DTYPE records with s_start absolute in the chunk, ops = the words
    they index. Returns (records[HIT_ROWS_DTYPE], rows[uint8])."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    m = np.ascontiguousarray(score_matrix, dtype=np.int32).reshape(-1)
    qid = np.ascontiguousarray(query_ids, dtype=np.uint32)
    p = np.ascontiguousarray(rec, dtype=HIT_PATH_DTYPE)
    w = np.ascontiguousarray(ops, dtype=np.uint32)
    if m.size != 32 * 32 or L <= 0 or qs.size % L or qid.shape != p.shape:
        raise ValueError("path_rows_host: bad argument shapes")
    n = len(qid)
    out = np.zeros(n, dtype=HIT_ROWS_DTYPE)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)

    def call(rows, cap, used):
        rc = lib.GhostmPathRowsHost(
            qs.ctypes.data_as(u8p), qs.size // L, L, dbs.ctypes.data_as(u8p), dbs.size,
            m.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n, qid.ctypes.data_as(u32p),
            p.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), w.ctypes.data_as(u32p), w.size, L, open_gap,
            extend_gap, out.ctypes.data_as(ctypes.POINTER(native.GhostmHitRows)), rows, cap, ctypes.byref(used))
        if rc != 0:
            raise GhostmError(native.last_error())

    used = ctypes.c_size_t(0)
    call(None, 0, used)  # the size needed
    rows = np.zeros(used.value, dtype=np.uint8)
    if used.value:
        call(rows.ctypes.data_as(u8p), used.value, used)
    return out, rows


def path_pileup_host(query_seqs, L, db, query_ids, rec, ops, profile=False):
    """The host model of the subject pile-up (GhostmPathPileupHost; no device):
    arguments as path_rows_host. Returns (depth, identities, consensus), each
    one element per residue of db, and with profile=True a fourth array of
    shape (len(db), 32)."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    qid = np.ascontiguousarray(query_ids, dtype=np.uint32)
    p = np.ascontiguousarray(rec, dtype=HIT_PATH_DTYPE)
    w = np.ascontiguousarray(ops, dtype=np.uint32)
    if L <= 0 or qs.size % L or qid.shape != p.shape:
        raise ValueError("path_pileup_host: bad argument shapes")
    depth = np.zeros(dbs.size, dtype=np.uint32)
    ident = np.zeros(dbs.size, dtype=np.uint32)
    cons = np.zeros(dbs.size, dtype=np.uint8)
    prof = np.zeros((dbs.size, 32), dtype=np.uint32) if profile else None
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    rc = lib.GhostmPathPileupHost(
        qs.ctypes.data_as(u8p), qs.size // L, L, dbs.ctypes.data_as(u8p), dbs.size, None, len(qid),
        qid.ctypes.data_as(u32p), p.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), w.ctypes.data_as(u32p), w.size,
        L, depth.ctypes.data_as(u32p), ident.ctypes.data_as(u32p), cons.ctypes.data_as(u8p),
        prof.ctypes.data_as(u32p) if profile else None)
    if rc != 0:
        raise GhostmError(native.last_error())
    return (depth, ident, cons, prof) if profile else (depth, ident, cons)


# GhostmSubjectReadPileup: SUBJECT_PILEUP_DTYPE's fields, then the summed shift columns
READ_PILEUP_DTYPE = np.dtype(SUBJECT_PILEUP_DTYPE.descr + [("shifts_sum", "<u8")])


def _read_pileup_call(fn, head, n_db, src, rec, ops, W, step, frame, tail, profile, shifts):
    """ReadPileupGpu and GhostmReadPileupHost take the same hit arguments and
    the same outputs."""
    srcs = np.ascontiguousarray(src, dtype=BAND_SOURCE_DTYPE)
    p = np.ascontiguousarray(rec, dtype=HIT_PATH_DTYPE)
    w = np.ascontiguousarray(ops, dtype=np.uint32)
    if srcs.shape != p.shape:
        raise ValueError("read pileup: bad argument shapes")
    depth = np.zeros(n_db, dtype=np.uint32)
    ident = np.zeros(n_db, dtype=np.uint32)
    cons = np.zeros(n_db, dtype=np.uint8)
    shf = np.zeros(n_db, dtype=np.uint32) if shifts else None
    prof = np.zeros((n_db, 32), dtype=np.uint32) if profile else None
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    rc = fn(*head, len(srcs), srcs.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
            p.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), w.ctypes.data_as(u32p), w.size, int(W), int(step),
            int(bool(frame)), *tail, depth.ctypes.data_as(u32p), ident.ctypes.data_as(u32p), cons.ctypes.data_as(u8p),
            shf.ctypes.data_as(u32p) if shifts else None, prof.ctypes.data_as(u32p) if profile else None)
    if rc != 0:
        raise GhostmError(native.last_error())
    return (depth, ident, cons, shf, prof)


def read_pileup_host(query_seqs, W, db, src, rec, ops, step, frame=False, profile=False, shifts=True):
    """The host model of the read-level pile-up (GhostmReadPileupHost; no
    device): query_seqs, db, src, rec, ops, step and frame as read_rows_host.
    Returns (depth, identities, consensus, shifts, profile), each one element
    per residue of db, profile of shape (len(db), 32); shifts and profile are
    None unless asked for."""
    lib = native.load()
    qs = np.ascontiguousarray(query_seqs, dtype=np.uint8).reshape(-1)
    dbs = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
    if W <= 0 or qs.size % W:
        raise ValueError("read_pileup_host: bad argument shapes")
    u8p = ctypes.POINTER(ctypes.c_uint8)
    head = (qs.ctypes.data_as(u8p), qs.size // W, int(W), dbs.ctypes.data_as(u8p), dbs.size)
    return _read_pileup_call(lib.GhostmReadPileupHost, head, dbs.size, src, rec, ops, W, step, frame, (), profile,
                             shifts)


def read_pileup(src, rec, ops, W, step, db_len, frame=False, profile=False, shifts=True):
    """ReadPileupGpu on the chunks of SetQueryGpu / SetDbGpu; db_len is the
    resident DB chunk's length; result as read_pileup_host."""
    lib = native.load()
    return _read_pileup_call(lib.ReadPileupGpu, (), int(db_len), src, rec, ops, W, step, frame, (int(db_len),),
                             profile, shifts)


def stage_read_pileup_stats() -> dict:
    """The read-level pile-up counters behind the stage-level calls (GhostmStageReadPileupStats)."""
    lib = native.load()
    st = native.GhostmReadPileupStats()
    lib.GhostmStageReadPileupStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmCullHit and GhostmCullOut (include/ghostm_hip.h)
CULL_HIT_DTYPE = np.dtype([("subject", "<u4"), ("score", "<u4"), ("q_lo", "<u4"), ("q_hi", "<u4"), ("s_lo", "<u4"),
                           ("s_hi", "<u4")])
CULL_OUT_DTYPE = np.dtype([("order", "<u4"), ("status", "<u4"), ("kept_rank", "<u4"), ("detail", "<u4")])
CULL_KEPT, CULL_DUP, CULL_CULLED, CULL_EMPTY = 0, 1, 2, 3


def _read_cull_call(fn, read_begin, hits, top_k, cover_pct, out):
    """ReadCullGpu and GhostmReadCullHost take the same arguments. out: the
    array the records go to (the refusal tests pass their own), or None."""
    rb = np.ascontiguousarray(read_begin, dtype=np.uint32).reshape(-1)
    h = np.ascontiguousarray(hits, dtype=CULL_HIT_DTYPE).reshape(-1)
    if out is None:
        out = np.zeros(len(h), dtype=CULL_OUT_DTYPE)
    if out.dtype != CULL_OUT_DTYPE or not out.flags.c_contiguous or len(out) < len(h):
        raise ValueError("read cull: out must be contiguous CULL_OUT_DTYPE records, one per hit")
    rc = fn(max(len(rb), 1) - 1, rb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if len(rb) else None, len(h),
            h.ctypes.data_as(ctypes.POINTER(native.GhostmCullHit)) if len(h) else None, int(top_k), int(cover_pct),
            out.ctypes.data_as(ctypes.POINTER(native.GhostmCullOut)) if len(out) else None)
    if rc != 0:
        raise GhostmError(native.last_error())
    return out


def read_cull_host(read_begin, hits, top_k=1, cover_pct=50, out=None):
    """The host model of the read-level cull (GhostmReadCullHost; no device):
    read r's hits are hits[read_begin[r]:read_begin[r + 1]] (CULL_HIT_DTYPE).
    Returns one CULL_OUT_DTYPE record per hit; hits outside every read keep
    out's bytes (zeros unless out is given)."""
    return _read_cull_call(native.load().GhostmReadCullHost, read_begin, hits, top_k, cover_pct, out)


def read_cull(read_begin, hits, top_k=1, cover_pct=50, out=None):
    """ReadCullGpu (k_read_cull); arguments and result as read_cull_host. Needs
    no resident chunk."""
    return _read_cull_call(native.load().ReadCullGpu, read_begin, hits, top_k, cover_pct, out)


def stage_read_cull_stats() -> dict:
    """The cull counters behind the stage-level calls (GhostmStageReadCullStats)."""
    lib = native.load()
    st = native.GhostmReadCullStats()
    lib.GhostmStageReadCullStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmLcaHit and GhostmLcaOut (include/ghostm_hip.h)
LCA_HIT_DTYPE = np.dtype([("node", "<u4"), ("score", "<u4"), ("q_lo", "<u4"), ("q_hi", "<u4")])
LCA_OUT_DTYPE = np.dtype([("node", "<u4"), ("depth", "<u4"), ("votes", "<u4"), ("support", "<u4"), ("lca", "<u4"),
                          ("candidates", "<u4"), ("unmapped", "<u4"), ("best_score", "<u4")])
_U32P = ctypes.POINTER(ctypes.c_uint32)


def taxonomy_depths(parent) -> np.ndarray:
    """The depths of a taxonomy given as parent indices (GhostmTaxonomyDepths;
    no device): checked as SetTaxonomyGpu checks it."""
    par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
    depth = np.zeros(len(par), dtype=np.uint32)
    if native.load().GhostmTaxonomyDepths(len(par), par.ctypes.data_as(_U32P) if len(par) else None,
                                          depth.ctypes.data_as(_U32P) if len(par) else None) != 0:
        raise GhostmError(native.last_error())
    return depth


def set_taxonomy_gpu(parent) -> None:
    """Makes the taxonomy resident for read_lca() (SetTaxonomyGpu); it stays
    until the next call or FreeGpu. A refused call keeps the previous one."""
    par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
    if native.load().SetTaxonomyGpu(len(par), par.ctypes.data_as(_U32P) if len(par) else None) != 0:
        raise GhostmError(native.last_error())


def _read_lca_args(read_begin, hits, top_pct, support_pct, out):
    rb = np.ascontiguousarray(read_begin, dtype=np.uint32).reshape(-1)
    h = np.ascontiguousarray(hits, dtype=LCA_HIT_DTYPE).reshape(-1)
    nreads = max(len(rb), 1) - 1
    if out is None:
        out = np.zeros(nreads, dtype=LCA_OUT_DTYPE)
    if out.dtype != LCA_OUT_DTYPE or not out.flags.c_contiguous or len(out) < nreads:
        raise ValueError("read lca: out must be contiguous LCA_OUT_DTYPE records, one per read")
    args = (nreads, rb.ctypes.data_as(_U32P) if len(rb) else None, len(h),
            h.ctypes.data_as(ctypes.POINTER(native.GhostmLcaHit)) if len(h) else None, int(top_pct), int(support_pct),
            out.ctypes.data_as(ctypes.POINTER(native.GhostmLcaOut)) if len(out) else None)
    return args, out, (rb, h)


def read_lca_host(parent, read_begin, hits, top_pct=10, support_pct=100, out=None):
    """The host model of the per-read taxonomic assignment (GhostmReadLcaHost;
    no device) over the taxonomy `parent`: read r's hits are
    hits[read_begin[r]:read_begin[r + 1]] (LCA_HIT_DTYPE). Returns one
    LCA_OUT_DTYPE record per read."""
    par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
    args, out, _keep = _read_lca_args(read_begin, hits, top_pct, support_pct, out)
    if native.load().GhostmReadLcaHost(len(par), par.ctypes.data_as(_U32P) if len(par) else None, *args) != 0:
        raise GhostmError(native.last_error())
    return out


def read_lca(read_begin, hits, top_pct=10, support_pct=100, out=None):
    """ReadLcaGpu (k_read_lca_wave, k_read_lca) over the taxonomy of
    set_taxonomy_gpu(); arguments and result as read_lca_host. Needs no
    resident chunk."""
    args, out, _keep = _read_lca_args(read_begin, hits, top_pct, support_pct, out)
    if native.load().ReadLcaGpu(*args) != 0:
        raise GhostmError(native.last_error())
    return out


def stage_read_lca_stats() -> dict:
    """The assignment's counters behind the stage-level calls (GhostmStageReadLcaStats)."""
    lib = native.load()
    st = native.GhostmReadLcaStats()
    lib.GhostmStageReadLcaStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmPairHit and GhostmPairOut (include/ghostm_hip.h)
PAIR_HIT_DTYPE = np.dtype([("subject", "<u4"), ("node", "<u4"), ("score", "<u4"), ("q_lo", "<u4"), ("q_hi", "<u4"),
                           ("s_lo", "<u4"), ("s_hi", "<u4"), ("strand", "<u4")])
PAIR_OUT_DTYPE = np.dtype([("joined", "<u4"), ("mates", "<u4"), ("best_score", "<u4"), ("best_span", "<u4")])


def _pair_join_call(fn, pair_begin, offset, hits, max_span, orient, out):
    """PairJoinGpu and GhostmPairJoinHost take the same arguments. out: the
    (cand, partner, pairs) arrays the results go to (the refusal tests pass
    their own), or None."""
    pb = np.ascontiguousarray(pair_begin, dtype=np.uint32).reshape(-1)
    off = np.ascontiguousarray(offset, dtype=np.uint32).reshape(-1)
    h = np.ascontiguousarray(hits, dtype=PAIR_HIT_DTYPE).reshape(-1)
    npairs = (max(len(pb), 1) - 1) // 2
    if len(pb) not in (0, 2 * npairs + 1) or len(off) != npairs:
        raise ValueError("pair join: pair_begin has 2 * npairs + 1 entries and offset npairs")
    if out is None:
        out = (np.zeros(len(h), dtype=LCA_HIT_DTYPE), np.full(len(h), 0xFFFFFFFF, dtype=np.uint32),
               np.zeros(npairs, dtype=PAIR_OUT_DTYPE))
    cand, partner, pairs = out
    if (cand.dtype != LCA_HIT_DTYPE or partner.dtype != np.uint32 or pairs.dtype != PAIR_OUT_DTYPE
            or not (cand.flags.c_contiguous and partner.flags.c_contiguous and pairs.flags.c_contiguous)
            or len(cand) < len(h) or len(partner) < len(h) or len(pairs) < npairs):
        raise ValueError("pair join: out must be contiguous (LCA_HIT_DTYPE per hit, uint32 per hit, PAIR_OUT_DTYPE per pair)")
    rc = fn(npairs, pb.ctypes.data_as(_U32P) if len(pb) else None, off.ctypes.data_as(_U32P) if len(off) else None,
            len(h), h.ctypes.data_as(ctypes.POINTER(native.GhostmPairHit)) if len(h) else None, int(max_span),
            int(orient), cand.ctypes.data_as(ctypes.POINTER(native.GhostmLcaHit)) if len(cand) else None,
            partner.ctypes.data_as(_U32P) if len(partner) else None,
            pairs.ctypes.data_as(ctypes.POINTER(native.GhostmPairOut)) if len(pairs) else None)
    if rc != 0:
        raise GhostmError(native.last_error())
    return cand, partner, pairs


def pair_join_host(pair_begin, offset, hits, max_span=1000, orient=0, out=None):
    """The host model of the mate-pair join (GhostmPairJoinHost; no device):
    pair p's hits are hits[pair_begin[2p]:pair_begin[2p + 1]] of mate 1 and
    hits[pair_begin[2p + 1]:pair_begin[2p + 2]] of mate 2 (PAIR_HIT_DTYPE),
    offset[p] mate 1's length. Returns (cand, partner, pairs): one
    LCA_HIT_DTYPE record and one partner index per hit, one PAIR_OUT_DTYPE
    record per pair; hits outside every pair keep out's bytes."""
    return _pair_join_call(native.load().GhostmPairJoinHost, pair_begin, offset, hits, max_span, orient, out)


def pair_join(pair_begin, offset, hits, max_span=1000, orient=0, out=None):
    """PairJoinGpu (k_pair_join); arguments and result as pair_join_host.
    Needs no resident chunk."""
    return _pair_join_call(native.load().PairJoinGpu, pair_begin, offset, hits, max_span, orient, out)


def stage_pair_join_stats() -> dict:
    """The join's counters behind the stage-level calls (GhostmStagePairJoinStats)."""
    lib = native.load()
    st = native.GhostmPairJoinStats()
    lib.GhostmStagePairJoinStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


# GhostmTaxonCount (include/ghostm_hip.h)
TAXON_COUNT_DTYPE = np.dtype([("node", "<u4"), ("clade_reads", "<u4"), ("direct_reads", "<u4"), ("kept_reads", "<u4")])


def _taxon_profile(call, name, nreads, node, min_reads, cap, with_final):
    """One profile call: the count first (cap 0, out NULL) unless cap is given,
    then the records. Returns (records, final nodes or None, summary dict)."""
    lib = native.load()
    min_reads = int(min_reads)
    if not 0 <= min_reads <= 0xFFFFFFFF:
        raise GhostmError(f"{name}: param: min_reads {min_reads} outside 1..2^32 - 1")
    nodep = node.ctypes.data_as(_U32P) if nreads else None
    nout = ctypes.c_size_t(0)
    if cap is None:
        if call(nreads, nodep, min_reads, 0, None, ctypes.byref(nout), None, None) != 0:
            raise GhostmError(native.last_error())
        cap = nout.value
    out = np.zeros(cap, dtype=TAXON_COUNT_DTYPE)
    final = np.zeros(nreads, dtype=np.uint32) if with_final else None
    summary = native.GhostmTaxonSummary()
    # a cap of 0 with a null out only counts: hand over a record's room then
    room = out if cap else np.zeros(1, dtype=TAXON_COUNT_DTYPE)
    if call(nreads, nodep, min_reads, cap, room.ctypes.data_as(ctypes.POINTER(native.GhostmTaxonCount)), ctypes.byref(nout),
            final.ctypes.data_as(_U32P) if with_final and nreads else None, ctypes.byref(summary)) != 0:
        raise GhostmError(native.last_error())
    return out[:nout.value], final, {n: getattr(summary, n) for n, _ in summary._fields_}


def taxon_profile_host(parent, node, min_reads=1, cap=None, with_final=True):
    """The host model of a sample's taxon profile (GhostmTaxonProfileHost; no
    device) over the taxonomy `parent`: node[r] is read r's node index or
    0xFFFFFFFF. Returns (TAXON_COUNT_DTYPE records in ascending node index,
    every read's final node, the summary as a dict). cap None asks for the
    count first; a cap below the count is refused with "cap"."""
    par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
    nd = np.ascontiguousarray(node, dtype=np.uint32).reshape(-1)
    fn = native.load().GhostmTaxonProfileHost
    parp = par.ctypes.data_as(_U32P) if len(par) else None
    return _taxon_profile(lambda *a: fn(len(par), parp, *a), "taxon profile", len(nd), nd, min_reads, cap, with_final)


def taxon_profile(node, min_reads=1, cap=None, with_final=True):
    """TaxonProfileGpu (k_taxon_count, k_taxon_climb, k_taxon_floor,
    k_taxon_final, k_taxon_sort_*, k_taxon_emit) over the taxonomy of set_taxonomy_gpu();
    arguments and result as taxon_profile_host. Needs no resident chunk."""
    nd = np.ascontiguousarray(node, dtype=np.uint32).reshape(-1)
    return _taxon_profile(native.load().TaxonProfileGpu, "taxon profile", len(nd), nd, min_reads, cap, with_final)


def stage_taxon_profile_stats() -> dict:
    """The profile's counters behind the stage-level calls (GhostmStageTaxonProfileStats)."""
    lib = native.load()
    st = native.GhostmTaxonProfileStats()
    lib.GhostmStageTaxonProfileStats(ctypes.byref(st), ctypes.sizeof(st))
    return {n: getattr(st, n) for n, _ in st._fields_}


class Aligner:
    """reference class Aligner (aligner.h:63-92): Execute(argc, argv)."""

    def execute(self, argv: Sequence[str]) -> int:
        lib = native.load()
        args = list(argv)
        return int(lib.GhostmAlignMain(len(args), native.argv_array(args)))


class Session:
    """`shard=(rank, world)`: search only that shard of the query set (one process
    per GPU, GhostmSessionCreateShard); rank-order concatenation of the shards'
    outputs is the unsharded output.

    `exchange`: an all-gather `f(send: bytes, sizes: list[int]) -> bytes` over
    the ranks (ghostm_amd.shard.torch_allgather): the shard then reads and
    counts only its own queries, and the ranks agree on the unsharded batch
    plan through it (GhostmSessionCreateShardEx). Without it, the shard counts
    every query of the set itself."""

    def __init__(self, argv: Sequence[str], shard: tuple[int, int] | None = None, exchange=None):
        lib = native.load()
        args = ["aln"] + list(argv)
        self._argv = native.argv_array(args)
        if shard is None:
            self._h = lib.GhostmSessionCreate(len(args), self._argv)
        elif exchange is None:
            self._h = lib.GhostmSessionCreateShard(len(args), self._argv, int(shard[0]), int(shard[1]))
        else:
            world = int(shard[1])
            errors = []

            def gather(_ctx, send, nbytes, recv, recv_bytes):
                try:
                    sizes = [int(recv_bytes[r]) for r in range(world)]
                    data = ctypes.string_at(send, nbytes) if nbytes else b""
                    out = exchange(data, sizes)
                    if len(out) != sum(sizes):
                        raise GhostmError(f"all-gather returned {len(out)} bytes, expected {sum(sizes)}")
                    if out:
                        ctypes.memmove(recv, out, len(out))
                    return 0
                except BaseException as e:  # noqa: BLE001 (reported through the C ABI)
                    errors.append(e)
                    return 1

            fn = native.ALLGATHER_FN(gather)  # alive for the duration of the call
            self._h = lib.GhostmSessionCreateShardEx(len(args), self._argv, int(shard[0]), world,
                                                     ctypes.cast(fn, ctypes.c_void_p), None)
            if errors:
                raise errors[0]
        if not self._h:
            raise GhostmError(native.last_error())

    @classmethod
    def for_db(cls, argv: Sequence[str]) -> "Session":
        """A database session (GhostmSessionCreateDb): `aln`'s options without -i,
        -S and -L; the DB chunks are resident and the queries come from
        set_queries / set_queries_fasta, any number of times."""
        lib = native.load()
        self = cls.__new__(cls)
        args = ["aln"] + list(argv)
        self._argv = native.argv_array(args)
        self._h = lib.GhostmSessionCreateDb(len(args), self._argv)
        if not self._h:
            raise GhostmError(native.last_error())
        return self

    @classmethod
    def for_queries(cls, argv: Sequence[str]) -> "Session":
        """A session without a database (GhostmSessionCreateQueries): `aln`'s
        options without -d; -i is optional. The database comes from set_db /
        set_db_fasta, any number of times; the queries from -i or from
        set_queries / set_queries_fasta."""
        lib = native.load()
        self = cls.__new__(cls)
        args = ["aln"] + list(argv)
        self._argv = native.argv_array(args)
        self._h = lib.GhostmSessionCreateQueries(len(args), self._argv)
        if not self._h:
            raise GhostmError(native.last_error())
        return self

    def set_db(self, seqs: Sequence, names: Sequence, k: int = 4, chunk_mb: int = 0) -> None:
        """Replaces the database by these records (str or bytes letters and
        names): what `ghostm db -k k -l chunk_mb` would format from them, coded
        and indexed on the device (GhostmSessionSetDb). The last run's results
        are dropped; the queries stay."""
        if len(seqs) != len(names):
            raise ValueError("set_db: one name per sequence")
        as_bytes = lambda x: x.encode() if isinstance(x, str) else bytes(x)  # noqa: E731
        bseqs = [as_bytes(x) for x in seqs]
        bnames = [as_bytes(x) for x in names]
        if any(b"\n" in x for x in bnames):
            raise ValueError("set_db: a name holds a newline")
        n = len(bseqs)
        lengths = np.array([len(x) for x in bseqs], dtype=np.uint32)
        offsets = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.uint64)
        raw = np.frombuffer(b"".join(bseqs) or b"\0", dtype=np.uint8)
        raw_len = int(lengths.sum(dtype=np.uint64))
        name_buf = b"".join(x + b"\n" for x in bnames)
        rc = native.load().GhostmSessionSetDb(
            self._h, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), raw_len,
            offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), name_buf, len(name_buf), n, int(k),
            int(chunk_mb))
        if rc != 0:
            raise GhostmError(native.last_error())

    def set_db_fasta(self, path: str, k: int = 4, chunk_mb: int = 0) -> None:
        """set_db from a FASTA file, read as `ghostm db` reads it
        (GhostmSessionSetDbFasta)."""
        if native.load().GhostmSessionSetDbFasta(self._h, str(path).encode(), int(k), int(chunk_mb)) != 0:
            raise GhostmError(native.last_error())

    def db_chunks(self) -> list[dict]:
        """The resident DB chunks in order (GhostmSessionDbChunks): id, nseq, len,
        seed, kcl and npos of each, as its .inf and .ind headers hold them."""
        lib = native.load()
        n = lib.GhostmSessionDbChunks(self._h, None, 0)
        info = (native.GhostmDbChunkInfo * max(n, 1))()
        n = lib.GhostmSessionDbChunks(self._h, info, n) if n else 0
        return [{f: int(getattr(info[c], f)) for f, _ in native.GhostmDbChunkInfo._fields_} for c in range(n)]

    def db_records(self, chunk: int) -> np.ndarray:
        """The residues of one DB chunk (the bytes of its .seq file), copied
        back from the device."""
        lib = native.load()
        n = lib.GhostmSessionDbRecords(self._h, int(chunk), None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=np.uint8)
        if n:
            lib.GhostmSessionDbRecords(self._h, int(chunk), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n)
        return out

    def db_index(self, chunk: int) -> tuple[int, np.ndarray, np.ndarray]:
        """(seed, keys_count, positions) of one DB chunk's index (its .ind file),
        copied back from the device (GhostmSessionDbIndex)."""
        chunks = self.db_chunks()
        if not 0 <= int(chunk) < len(chunks):
            raise GhostmError(f"DB chunk {chunk} of {len(chunks)}")
        c = chunks[int(chunk)]
        kc = np.zeros(c["kcl"], dtype=np.uint32)
        pos = np.zeros(c["npos"], dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if native.load().GhostmSessionDbIndex(self._h, int(chunk), kc.ctypes.data_as(u32p), kc.size,
                                              pos.ctypes.data_as(u32p), pos.size) != 0:
            raise GhostmError(native.last_error())
        return c["seed"], kc, pos

    def set_queries(self, seqs: Sequence, names: Sequence, width: int = 75, dna: bool = False,
                    chunk_mb: int = 0, tile_step: int | None = None, max_len: int = 0, quals: Sequence | None = None) -> None:
        """Replaces the query set by these records (str or bytes letters and
        names): what `ghostm qry -l width [-t d] -L chunk_mb` would format from
        them, coded on the device (GhostmSessionSetQueries). The last run's
        results are dropped. With tile_step the set is tiled
        (GhostmSessionSetQueriesTiled): every record is cut at max_len (letters,
        nt for DNA; 0: no cut) and enters as overlapping tile records of the
        width, tile_step letters apart; query_tiles() gives the table. quals
        (tiled sets only): every record's quality bytes (Phred+33), as long as
        its letters; the set then goes through the quality stage of
        set_quality() (GhostmSessionSetQueriesQualTiled)."""
        if tile_step is None and max_len:
            raise ValueError("set_queries: max_len cuts a tiled set only (give tile_step)")
        if len(seqs) != len(names):
            raise ValueError("set_queries: one name per sequence")
        if quals is not None:
            if tile_step is None:
                raise ValueError("set_queries: quals go with a tiled set only (give tile_step)")
            if len(quals) != len(seqs) or any(len(q) != len(x) for q, x in zip(quals, seqs)):
                raise ValueError("set_queries: one quality byte per letter")
        as_bytes = lambda x: x.encode() if isinstance(x, str) else bytes(x)  # noqa: E731
        bseqs = [as_bytes(x) for x in seqs]
        bnames = [as_bytes(x) for x in names]
        if any(b"\n" in x for x in bnames):
            raise ValueError("set_queries: a name holds a newline")
        n = len(bseqs)
        lengths = np.array([len(x) for x in bseqs], dtype=np.uint32)
        offsets = np.zeros(n, dtype=np.uint64)
        if n > 1:
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.uint64)
        raw = np.frombuffer(b"".join(bseqs) or b"\0", dtype=np.uint8)
        raw_len = int(lengths.sum(dtype=np.uint64))
        name_buf = b"".join(x + b"\n" for x in bnames)
        args = (self._h, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), raw_len,
                offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), name_buf, len(name_buf), n, int(width),
                int(bool(dna)), int(chunk_mb))
        if quals is not None:
            qraw = np.frombuffer(b"".join(as_bytes(q) for q in quals) or b"\0", dtype=np.uint8)
            u8p = ctypes.POINTER(ctypes.c_uint8)
            rc = native.load().GhostmSessionSetQueriesQualTiled(args[0], args[1], qraw.ctypes.data_as(u8p), *args[2:],
                                                                int(max_len), int(tile_step))
        elif tile_step is None:
            rc = native.load().GhostmSessionSetQueries(*args)
        else:
            rc = native.load().GhostmSessionSetQueriesTiled(*args, int(max_len), int(tile_step))
        if rc != 0:
            raise GhostmError(native.last_error())

    def set_queries_fasta(self, path: str, width: int = 75, dna: bool = False, chunk_mb: int = 0,
                          tile_step: int | None = None, max_len: int = 0) -> int:
        """set_queries from a FASTA file, read as `ghostm qry` reads it
        (GhostmSessionSetQueriesFasta). Returns the number of output records
        over the width (qry's warnings). With tile_step the set is tiled
        (GhostmSessionSetQueriesFastaTiled) and the count is of the records
        max_len cut (six per DNA read)."""
        if tile_step is None and max_len:
            raise ValueError("set_queries_fasta: max_len cuts a tiled set only (give tile_step)")
        cut = ctypes.c_uint64(0)
        if tile_step is None:
            rc = native.load().GhostmSessionSetQueriesFasta(self._h, str(path).encode(), int(width), int(bool(dna)),
                                                            int(chunk_mb), ctypes.byref(cut))
        else:
            rc = native.load().GhostmSessionSetQueriesFastaTiled(self._h, str(path).encode(), int(width),
                                                                 int(bool(dna)), int(chunk_mb), int(max_len),
                                                                 int(tile_step), ctypes.byref(cut))
        if rc != 0:
            raise GhostmError(native.last_error())
        return int(cut.value)

    def set_quality(self, trim: int = 20, mask: int = 0, min_len: int = 0) -> None:
        """Quality trimming and masking of the FASTQ and quality-carrying sets
        made from now on (GhostmSessionSetQuality): both ends trimmed by BWA's
        running sum at quality `trim`, kept letters below `mask` stored as N,
        reads left shorter than min_len emptied (they stay as records).
        set_quality(0, 0, 0) turns it off (the default). A refusal ("param")
        leaves the old setting."""
        args = [int(trim), int(mask), int(min_len)]
        if any(not 0 <= v < 1 << 32 for v in args):  # beyond the C arguments' range
            raise GhostmError("quality: param: an argument beyond 32 bits")
        if native.load().GhostmSessionSetQuality(self._h, *args) != 0:
            raise GhostmError(native.last_error())

    def set_adapters(self, adapter1: str = "", adapter2: str = "", min_overlap: int = 5, err_pct: int = 10,
                     pair_overlap: int = 0) -> None:
        """Adapter removal on the FASTQ and quality-carrying DNA sets made from
        now on (GhostmSessionSetAdapters), ahead of the quality stage: adapter1
        (adapter2 in the odd records, when given) is looked for at every read's
        3' end with at least min_overlap letters and at most err_pct % of
        mismatches, and with pair_overlap > 0 (20 or more is sensible) records
        2i and 2i + 1 are mates whose read-through is cut at their overlap.
        set_adapters() turns it off (the default). A refusal ("param",
        "adapter") leaves the old setting."""
        args = [int(min_overlap), int(err_pct), int(pair_overlap)]
        if any(not 0 <= v < 1 << 32 for v in args):  # beyond the C arguments' range
            raise GhostmError("adapters: param: an argument beyond 32 bits")
        if native.load().GhostmSessionSetAdapters(self._h, _adapter_text(adapter1), _adapter_text(adapter2), *args) != 0:
            raise GhostmError(native.last_error())

    def query_adapters(self) -> np.ndarray:
        """One ADAPTER_OUT_DTYPE record per source read of the current set
        (GhostmSessionQueryAdapters); empty when the adapter stage did not run."""
        lib = native.load()
        n = lib.GhostmSessionQueryAdapters(self._h, None, 0)
        out = np.zeros(n, dtype=ADAPTER_OUT_DTYPE)
        if n:
            lib.GhostmSessionQueryAdapters(self._h, out.ctypes.data_as(ctypes.POINTER(native.GhostmAdapterOut)), n)
        return out

    def adapter_stats(self) -> dict:
        """The adapter counters of the current query set (GhostmSessionAdapterStats)."""
        st = native.GhostmAdapterStats()
        native.load().GhostmSessionAdapterStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {n: getattr(st, n) for n, _ in st._fields_}

    def set_queries_fastq(self, path: str, width: int = 75, dna: bool = False, chunk_mb: int = 0,
                          tile_step: int = 64, max_len: int = 0) -> int:
        """The tiled set_queries_fasta from a four-line FASTQ file, through the
        quality stage of set_quality() (GhostmSessionSetQueriesFastqTiled).
        Read coordinates in every result are relative to the kept stretch;
        query_quality()["begin"] converts them back."""
        cut = ctypes.c_uint64(0)
        rc = native.load().GhostmSessionSetQueriesFastqTiled(self._h, str(path).encode(), int(width), int(bool(dna)),
                                                             int(chunk_mb), int(max_len), int(tile_step),
                                                             ctypes.byref(cut))
        if rc != 0:
            raise GhostmError(native.last_error())
        return int(cut.value)

    def set_queries_fastq_mates(self, path1: str, path2: str, width: int = 75, dna: bool = False, chunk_mb: int = 0,
                                tile_step: int = 64, max_len: int = 0) -> int:
        """set_queries_fastq over two files of mates, interleaved record by
        record (GhostmSessionSetQueriesFastqMatesTiled); a mate the quality
        stage empties stays a record."""
        cut = ctypes.c_uint64(0)
        rc = native.load().GhostmSessionSetQueriesFastqMatesTiled(
            self._h, str(path1).encode(), str(path2).encode(), int(width), int(bool(dna)), int(chunk_mb), int(max_len),
            int(tile_step), ctypes.byref(cut))
        if rc != 0:
            raise GhostmError(native.last_error())
        return int(cut.value)

    def query_quality(self) -> np.ndarray:
        """One QUAL_OUT_DTYPE record per source read of the current set
        (GhostmSessionQueryQuality); empty when the quality stage did not run."""
        lib = native.load()
        n = lib.GhostmSessionQueryQuality(self._h, None, 0)
        out = np.zeros(n, dtype=QUAL_OUT_DTYPE)
        if n:
            lib.GhostmSessionQueryQuality(self._h, out.ctypes.data_as(ctypes.POINTER(native.GhostmQualOut)), n)
        return out

    def quality_stats(self) -> dict:
        """The quality counters of the current query set (GhostmSessionQualityStats)."""
        st = native.GhostmQualStats()
        native.load().GhostmSessionQualityStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {n: getattr(st, n) for n, _ in st._fields_}

    def query_tiles(self) -> np.ndarray:
        """The tile table of a tiled query set (GhostmSessionQueryTiles): one
        QUERY_TILE_DTYPE entry per query record over the chunks in order, the
        indexing of query_lengths() and of hits_rows()'s query_record; empty on
        an untiled set."""
        lib = native.load()
        n = lib.GhostmSessionQueryTiles(self._h, None, 0)
        out = np.zeros(n, dtype=QUERY_TILE_DTYPE)
        if n:
            lib.GhostmSessionQueryTiles(self._h, out.ctypes.data_as(ctypes.POINTER(native.GhostmQueryTile)), n)
        return out

    def set_output(self, path: str) -> None:
        """The -o path of later run(to_file=True) and write() calls."""
        if native.load().GhostmSessionSetOutputFile(self._h, str(path).encode()) != 0:
            raise GhostmError(native.last_error())

    def query_lengths(self) -> np.ndarray:
        """The length `aln` prints for every query record (last non-X code + 1, at
        least 1), over the chunks in order."""
        lib = native.load()
        n = lib.GhostmSessionQueryLengths(self._h, None, 0)
        out = np.zeros(n, dtype=np.uint32)
        if n:
            lib.GhostmSessionQueryLengths(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n)
        return out

    def set_mask(self, window: int = 12, trigger: int = 220, extend: int = 250) -> None:
        """Low-complexity masking of the query sets made from now on
        (GhostmSessionSetMask): window 6..32 letters, trigger <= extend in
        hundredths of a bit, at most 500; set_mask(0) turns it off (the
        default). It takes effect at the next set_queries*; the current set
        stays as it is. A refusal ("window", "levels") leaves the old setting."""
        args = [int(window), int(trigger), int(extend)]
        if any(not 0 <= v < 1 << 32 for v in args):  # beyond the C arguments' range
            raise GhostmError("mask: window: or levels: an argument beyond 32 bits")
        if native.load().GhostmSessionSetMask(self._h, *args) != 0:
            raise GhostmError(native.last_error())

    def query_masked(self) -> np.ndarray:
        """The letters masked in every query record, indexed as query_lengths()
        (GhostmSessionQueryMasked); empty for a set made with masking off."""
        lib = native.load()
        n = lib.GhostmSessionQueryMasked(self._h, None, 0)
        out = np.zeros(n, dtype=np.uint32)
        if n:
            lib.GhostmSessionQueryMasked(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n)
        return out

    def mask_stats(self) -> dict:
        """The mask counters of the current query set (GhostmSessionMaskStats)."""
        st = native.GhostmMaskStats()
        native.load().GhostmSessionMaskStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {n: getattr(st, n) for n, _ in st._fields_}

    def query_records(self, chunk: int) -> np.ndarray:
        """The coded records of one query chunk (the bytes of its .seq file),
        copied back from the device."""
        lib = native.load()
        n = lib.GhostmSessionQueryRecords(self._h, int(chunk), None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=np.uint8)
        if n:
            lib.GhostmSessionQueryRecords(self._h, int(chunk), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n)
        return out

    def shard_range(self) -> tuple[int, int]:
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        native.load().GhostmSessionShardRange(self._h, ctypes.byref(b), ctypes.byref(e))
        return b.value, e.value

    def hit_capacity(self) -> int:
        """The most hit records one run can return (name groups x max(-b, 1),
        GhostmSessionHitCapacity): the size of a fixed gather buffer."""
        return int(native.load().GhostmSessionHitCapacity(self._h))

    def run(self, to_file: bool = False) -> None:
        """The search; to_file also writes the -o file while it runs
        (GhostmSessionRunToFile), after which write() is a no-op."""
        lib = native.load()
        rc = lib.GhostmSessionRunToFile(self._h) if to_file else lib.GhostmSessionRun(self._h)
        if rc != 0:
            raise GhostmError(native.last_error())

    def output(self) -> bytes:
        lib = native.load()
        n = lib.GhostmSessionOutput(self._h, None, 0)
        buf = ctypes.create_string_buffer(n)
        lib.GhostmSessionOutput(self._h, buf, n)
        return buf.raw[:n]

    def write(self) -> None:
        if native.load().GhostmSessionWrite(self._h) != 0:
            raise GhostmError(native.last_error())

    def hits(self) -> np.ndarray:
        lib = native.load()
        n = lib.GhostmSessionHits(self._h, None, 0)
        out = np.zeros(n, dtype=HIT_DTYPE)
        if n:
            lib.GhostmSessionHits(self._h, out.ctypes.data_as(ctypes.POINTER(native.GhostmHit)), n)
        return out

    def hits_ext(self) -> np.ndarray:
        """One HIT_EXT_DTYPE record per hit of hits() (GhostmSessionHitsExt): query
        coordinates, mismatches and gap opens, after a run with any -y."""
        lib = native.load()
        n = lib.GhostmSessionHitsExt(self._h, None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=HIT_EXT_DTYPE)
        if n:
            lib.GhostmSessionHitsExt(self._h, out.ctypes.data_as(ctypes.POINTER(native.GhostmHitExt)), n)
        return out

    def hits_path(self) -> tuple[np.ndarray, np.ndarray]:
        """(records, ops): one HIT_PATH_DTYPE record per hit of hits()
        (GhostmSessionHitsPath) and the run-length words they index
        (GhostmSessionPathOps), after a run with any -y. cigar(ops[o:o + n]) is
        a hit's extended CIGAR."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionHitsPath(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=HIT_PATH_DTYPE)
        if n:
            lib.GhostmSessionHitsPath(self._h, rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), n)
        m = lib.GhostmSessionPathOps(self._h, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        ops = np.zeros(m, dtype=np.uint32)
        if m:
            lib.GhostmSessionPathOps(self._h, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m)
        return rec, ops

    def hits_band(self) -> tuple[np.ndarray, np.ndarray]:
        """(records, ops): one read-level HIT_PATH_DTYPE record per hit of hits()
        (GhostmSessionHitsBand) and the run-length words they index
        (GhostmSessionBandOps), after a run with any -y: the whole read or
        frame aligned to the whole subject inside a band around the hit's tile
        path. q_start / q_end are read or frame coordinates; cigar() works on
        the words."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionHitsBand(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=HIT_PATH_DTYPE)
        if n:
            lib.GhostmSessionHitsBand(self._h, rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), n)
        m = lib.GhostmSessionBandOps(self._h, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        ops = np.zeros(m, dtype=np.uint32)
        if m:
            lib.GhostmSessionBandOps(self._h, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m)
        return rec, ops

    def set_band(self, band: int) -> None:
        """The half-width of hits_band()'s band, 1..31 (default 31). A refusal
        leaves the old value; a change drops the kept band results."""
        b = int(band)
        if not 0 <= b < 1 << 32:  # beyond the C argument's range
            raise GhostmError(f"band: half-width {b} outside 1..31")
        if native.load().GhostmSessionSetBand(self._h, b) != 0:
            raise GhostmError(native.last_error())

    def hits_frame(self) -> tuple[np.ndarray, np.ndarray]:
        """(records, ops): one frameshift-aware read-level HIT_PATH_DTYPE record
        per hit of hits() (GhostmSessionHitsFrame) and the run-length words they
        index (GhostmSessionFrameOps; op codes 0..5, frame_cigar() prints
        them), after a run with any -y on a DNA set of a tiled setter. q_start
        / q_end are strand positions in nucleotides."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionHitsFrame(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=HIT_PATH_DTYPE)
        if n:
            lib.GhostmSessionHitsFrame(self._h, rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), n)
        return rec, self.frame_ops()

    def frame_ops(self) -> np.ndarray:
        """The run-length words of hits_frame()'s records (GhostmSessionFrameOps)."""
        lib = native.load()
        m = lib.GhostmSessionFrameOps(self._h, None, 0)
        if m == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        ops = np.zeros(m, dtype=np.uint32)
        if m:
            lib.GhostmSessionFrameOps(self._h, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), m)
        return ops

    def frame_info(self) -> np.ndarray:
        """One HIT_FRAME_INFO_DTYPE record per hit (GhostmSessionFrameInfo):
        strand, the read's kept nucleotides, the frames' letters, the shifts."""
        lib = native.load()
        n = lib.GhostmSessionFrameInfo(self._h, None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        info = np.zeros(n, dtype=HIT_FRAME_INFO_DTYPE)
        if n:
            lib.GhostmSessionFrameInfo(self._h, info.ctypes.data_as(ctypes.POINTER(native.GhostmHitFrameInfo)), n)
        return info

    def set_frame_shift(self, shift_cost: int) -> None:
        """The frameshift cost of hits_frame(), -(1 << 20)..0 (default -15). A
        refusal leaves the old value; a change drops the kept frame results."""
        v = int(shift_cost)
        if not -(1 << 31) <= v < 1 << 31:  # beyond the C argument's range
            raise GhostmError(f"shift: frameshift cost {v} outside -(1 << 20)..0")
        if native.load().GhostmSessionSetFrameShift(self._h, v) != 0:
            raise GhostmError(native.last_error())

    def frame_stats(self) -> dict:
        """The frame pass's counters since the last run (GhostmSessionFrameStats)."""
        st = native.GhostmFrameStats()
        native.load().GhostmSessionFrameStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def _read_rows(self, hits_fn, bytes_fn) -> tuple[np.ndarray, np.ndarray]:
        bad = ctypes.c_size_t(-1).value
        n = hits_fn(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=READ_ROWS_DTYPE)
        if n:
            hits_fn(self._h, rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)), n)
        m = bytes_fn(self._h, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        rows = np.zeros(m, dtype=np.uint8)
        if m:
            bytes_fn(self._h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m)
        return rec, rows

    def hits_band_rows(self) -> tuple[np.ndarray, np.ndarray]:
        """(records, rows): one READ_ROWS_DTYPE record per hit of hits() for its
        read-level path (hits_band()) and the row bytes they index
        (GhostmSessionHitsBandRows, GhostmSessionBandRowBytes), after a run with
        any -y. rows_of(rec, rows, h) is hit h's three rows."""
        lib = native.load()
        return self._read_rows(lib.GhostmSessionHitsBandRows, lib.GhostmSessionBandRowBytes)

    def hits_frame_rows(self) -> tuple[np.ndarray, np.ndarray]:
        """The same for the frame paths (hits_frame()): the query row holds '\\'
        and '/' at the frameshifts (GhostmSessionHitsFrameRows,
        GhostmSessionFrameRowBytes). Refused where hits_frame() is."""
        lib = native.load()
        return self._read_rows(lib.GhostmSessionHitsFrameRows, lib.GhostmSessionFrameRowBytes)

    def read_rows_stats(self) -> dict:
        """The read-rows counters since the last run (GhostmSessionReadRowsStats)."""
        st = native.GhostmReadRowsStats()
        native.load().GhostmSessionReadRowsStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def hits_rows(self) -> tuple[np.ndarray, np.ndarray]:
        """(records, rows): one HIT_ROWS_DTYPE record per hit of hits()
        (GhostmSessionHitsRows) and the row bytes they index
        (GhostmSessionRowBytes), after a run with any -y. rows_of(rec, rows, h)
        is hit h's (query row, midline, subject row)."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionHitsRows(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=HIT_ROWS_DTYPE)
        if n:
            lib.GhostmSessionHitsRows(self._h, rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitRows)), n)
        m = lib.GhostmSessionRowBytes(self._h, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        rows = np.zeros(m, dtype=np.uint8)
        if m:
            lib.GhostmSessionRowBytes(self._h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m)
        return rec, rows

    def pileup(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(subjects, depth, identities, consensus): one SUBJECT_PILEUP_DTYPE
        record per subject in db_id order (GhostmSessionPileup) and the
        subjects' positions concatenated (GhostmSessionPileupArrays); subject i
        is [offset, offset + length). After a run with any -y."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionPileup(self._h, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        subj = np.zeros(n, dtype=SUBJECT_PILEUP_DTYPE)
        if n:
            lib.GhostmSessionPileup(self._h, subj.ctypes.data_as(ctypes.POINTER(native.GhostmSubjectPileup)), n)
        m = lib.GhostmSessionPileupArrays(self._h, None, None, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        depth = np.zeros(m, dtype=np.uint32)
        ident = np.zeros(m, dtype=np.uint32)
        cons = np.full(m, 255, dtype=np.uint8)
        if m:
            u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.GhostmSessionPileupArrays(self._h, depth.ctypes.data_as(u32p), ident.ctypes.data_as(u32p),
                                          cons.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m)
        return subj, depth, ident, cons

    def subject_profile(self, db_id: int) -> np.ndarray:
        """The 32-slot rows of subject db_id, shape (length, 32)
        (GhostmSessionSubjectProfile): made on demand, nothing is kept."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        n = lib.GhostmSessionSubjectProfile(self._h, db_id, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        prof = np.zeros(n, dtype=np.uint32)
        if n and lib.GhostmSessionSubjectProfile(self._h, db_id, prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                 n) == bad:
            raise GhostmError(native.last_error())
        return prof.reshape(-1, 32)

    def read_pileup(self, frame: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(subjects, depth, identities, consensus, shifts): pileup() from the
        read-level paths, hits_band()'s (frame False) or hits_frame()'s (frame
        True): one READ_PILEUP_DTYPE record per subject (GhostmSessionReadPileup)
        and the subjects' positions concatenated
        (GhostmSessionReadPileupArrays). frame=True is refused where
        hits_frame() is."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionReadPileup(self._h, f, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        subj = np.zeros(n, dtype=READ_PILEUP_DTYPE)
        if n:
            lib.GhostmSessionReadPileup(self._h, f, subj.ctypes.data_as(ctypes.POINTER(native.GhostmSubjectReadPileup)), n)
        m = lib.GhostmSessionReadPileupArrays(self._h, f, None, None, None, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        depth = np.zeros(m, dtype=np.uint32)
        ident = np.zeros(m, dtype=np.uint32)
        cons = np.full(m, 255, dtype=np.uint8)
        shifts = np.zeros(m, dtype=np.uint32)
        if m:
            u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.GhostmSessionReadPileupArrays(self._h, f, depth.ctypes.data_as(u32p), ident.ctypes.data_as(u32p),
                                              cons.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                              shifts.ctypes.data_as(u32p), m)
        return subj, depth, ident, cons, shifts

    def read_cull(self, frame: bool = False) -> np.ndarray:
        """One CULL_OUT_DTYPE record per hit of hits() (GhostmSessionReadCull):
        the hits of every read ranked by the read-level score of hits_band()
        (frame False) or hits_frame() (frame True), with the hits that repeat a
        kept alignment (CULL_DUP, detail = the kept hit's index in hits()) and
        the hits whose stretch of the read kept hits cover (CULL_CULLED) marked.
        Computed on first use. frame=True is refused where hits_frame() is."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionReadCull(self._h, f, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=CULL_OUT_DTYPE)
        if n and lib.GhostmSessionReadCull(self._h, f, out.ctypes.data_as(ctypes.POINTER(native.GhostmCullOut)),
                                           n) == bad:
            raise GhostmError(native.last_error())
        return out

    def set_cull(self, top_k: int = 1, cover_pct: int = 50) -> None:
        """read_cull()'s parameters: a hit is culled when top_k (1..255) kept
        hits cover cover_pct (1..100) per cent of its stretch of the read. A
        refusal leaves the old values; a change drops the kept result."""
        k, pct = int(top_k), int(cover_pct)
        if not (0 <= k < 1 << 32 and 0 <= pct < 1 << 32):  # beyond the C arguments' range
            raise GhostmError(f"cull: param: top_k {k}, cover_pct {pct} outside 1..255, 1..100")
        if native.load().GhostmSessionSetCull(self._h, k, pct) != 0:
            raise GhostmError(native.last_error())

    def read_cull_stats(self) -> dict:
        """The cull's counters since the last run (GhostmSessionReadCullStats)."""
        st = native.GhostmReadCullStats()
        native.load().GhostmSessionReadCullStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def set_tile_groups(self, on: bool = True) -> None:
        """From the next tiled setter on, keep the best -b hits per tile instead
        of per read (GhostmSessionSetTileGroups). Off by default; refused on a
        shard session."""
        if native.load().GhostmSessionSetTileGroups(self._h, int(bool(on))) != 0:
            raise GhostmError(native.last_error())

    def set_taxonomy(self, taxid, parent, subject_node) -> None:
        """A taxonomy for the resident database (GhostmSessionSetTaxonomy):
        taxid[i] labels node i (distinct, at least 1), parent[i] is its parent's
        index (the root its own), subject_node[db_id] a node or 0xFFFFFFFF. A
        refusal leaves the session as it was; set_db* drop the taxonomy."""
        tid = np.ascontiguousarray(taxid, dtype=np.uint32).reshape(-1)
        par = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
        sub = np.ascontiguousarray(subject_node, dtype=np.uint32).reshape(-1)
        if len(tid) != len(par):
            raise GhostmError("set taxonomy: taxonomy: taxid and parent differ in length")
        if native.load().GhostmSessionSetTaxonomy(self._h, len(par), tid.ctypes.data_as(_U32P) if len(tid) else None,
                                                  par.ctypes.data_as(_U32P) if len(par) else None, len(sub),
                                                  sub.ctypes.data_as(_U32P) if len(sub) else None) != 0:
            raise GhostmError(native.last_error())

    def set_taxonomy_files(self, nodes_path: str, map_path: str) -> None:
        """The same from a nodes file (taxid, parent taxid per line; NCBI's
        nodes.dmp reads as it is) and a map file (subject name, taxid)
        (GhostmSessionSetTaxonomyFiles)."""
        if native.load().GhostmSessionSetTaxonomyFiles(self._h, os.fsencode(nodes_path), os.fsencode(map_path)) != 0:
            raise GhostmError(native.last_error())

    def taxonomy_info(self) -> dict:
        """nodes (0: no taxonomy), subjects_mapped, subjects_unmapped and the
        map lines that matched no subject (GhostmSessionTaxonomyInfo)."""
        st = native.GhostmTaxonomyInfo()
        native.load().GhostmSessionTaxonomyInfo(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def set_lca(self, top_pct: int = 10, support_pct: int = 100) -> None:
        """read_lca()'s parameters: a kept hit votes when its score is within
        top_pct (0..100) per cent of the best on its stretch of the read; the
        taxon is the deepest node with support_pct (51..100) per cent of the
        votes. A refusal leaves the old values; a change drops the kept result."""
        top, sup = int(top_pct), int(support_pct)
        if not (0 <= top <= 100 and 51 <= sup <= 100):  # GhostmSessionSetLca's ranges; an int beyond uint32 would wrap
            raise GhostmError(f"lca: param: top_pct {top}, support_pct {sup} outside 0..100, 51..100")
        if native.load().GhostmSessionSetLca(self._h, top, sup) != 0:
            raise GhostmError(native.last_error())

    def read_lca(self, frame: bool = False, with_begin: bool = False):
        """One LCA_OUT_DTYPE record per read of read_cull(frame)
        (GhostmSessionReadLca): the taxon of the read from the hits the cull
        keeps. node and lca are node indices. with_begin: also every read's
        first hit as an index of hits(), plus the end. Computed on first use."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionReadLca(self._h, f, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=LCA_OUT_DTYPE)
        if n and lib.GhostmSessionReadLca(self._h, f, out.ctypes.data_as(ctypes.POINTER(native.GhostmLcaOut)), n) == bad:
            raise GhostmError(native.last_error())
        if not with_begin:
            return out
        begin = np.zeros(n + 1, dtype=np.uint32)
        if lib.GhostmSessionReadLcaBegin(self._h, f, begin.ctypes.data_as(_U32P), n + 1) == bad:
            raise GhostmError(native.last_error())
        return out, begin

    def read_lca_stats(self) -> dict:
        """The assignment's counters since the last run (GhostmSessionReadLcaStats)."""
        st = native.GhostmReadLcaStats()
        native.load().GhostmSessionReadLcaStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def set_mates(self, on: bool = True, max_insert: int = 1000) -> None:
        """Declares source records 2i and 2i + 1 of a tiled query set to be
        mates (GhostmSessionSetMates); max_insert is the longest fragment in
        read units (nt on a DNA set). Off by default. With mates on,
        taxon_profile() counts fragments. A change drops only the pair results."""
        m = int(max_insert)
        if not 1 <= m <= 1 << 24:  # GhostmSessionSetMates' range; an int beyond uint32 would wrap
            raise GhostmError(f"mates: param: max_insert {m} outside 1..2^24")
        if native.load().GhostmSessionSetMates(self._h, int(bool(on)), m) != 0:
            raise GhostmError(native.last_error())

    def set_queries_fasta_mates(self, path1: str, path2: str, width: int = 75, dna: bool = False, chunk_mb: int = 0,
                                tile_step: int = 64, max_len: int = 0) -> int:
        """The tiled set_queries_fasta over two files of mates, interleaved
        record by record (GhostmSessionSetQueriesFastaMatesTiled). Files of
        different record counts are refused and leave the old set in place."""
        cut = ctypes.c_uint64(0)
        rc = native.load().GhostmSessionSetQueriesFastaMatesTiled(
            self._h, str(path1).encode(), str(path2).encode(), int(width), int(bool(dna)), int(chunk_mb), int(max_len),
            int(tile_step), ctypes.byref(cut))
        if rc != 0:
            raise GhostmError(native.last_error())
        return int(cut.value)

    def pair_join(self, frame: bool = False):
        """The join of every pair's hits from read_cull(frame)
        (GhostmSessionPairJoin, GhostmSessionPairJoinPairs). Returns (cand,
        partner, pairs, pair_begin, pair_record): one LCA_HIT_DTYPE candidate
        and one partner (an index of hits(), or 0xFFFFFFFF) per hit, one
        PAIR_OUT_DTYPE record per pair with a hit, the pairs' borders in hits()
        (two per pair and the end) and mate 1's source record. Computed on
        first use."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionPairJoin(self._h, f, None, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        cand = np.zeros(n, dtype=LCA_HIT_DTYPE)
        partner = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        if n and lib.GhostmSessionPairJoin(self._h, f, cand.ctypes.data_as(ctypes.POINTER(native.GhostmLcaHit)),
                                           partner.ctypes.data_as(_U32P), n) == bad:
            raise GhostmError(native.last_error())
        m = lib.GhostmSessionPairJoinPairs(self._h, f, None, None, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        pairs = np.zeros(m, dtype=PAIR_OUT_DTYPE)
        begin = np.zeros(2 * m + 1, dtype=np.uint32)
        record = np.zeros(m, dtype=np.uint32)
        if lib.GhostmSessionPairJoinPairs(self._h, f, pairs.ctypes.data_as(ctypes.POINTER(native.GhostmPairOut)),
                                          begin.ctypes.data_as(_U32P), record.ctypes.data_as(_U32P), m) == bad:
            raise GhostmError(native.last_error())
        return cand, partner, pairs, begin, record

    def pair_lca(self, frame: bool = False) -> np.ndarray:
        """One LCA_OUT_DTYPE record per pair of pair_join(frame)
        (GhostmSessionPairLca): the taxon of the fragment from the joined
        candidates, under set_lca()'s parameters. Computed on first use."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionPairLca(self._h, f, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        out = np.zeros(n, dtype=LCA_OUT_DTYPE)
        if n and lib.GhostmSessionPairLca(self._h, f, out.ctypes.data_as(ctypes.POINTER(native.GhostmLcaOut)), n) == bad:
            raise GhostmError(native.last_error())
        return out

    def pair_join_stats(self) -> dict:
        """The join's counters since the last run (GhostmSessionPairJoinStats)."""
        st = native.GhostmPairJoinStats()
        native.load().GhostmSessionPairJoinStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def set_profile(self, min_reads: int = 1) -> None:
        """taxon_profile()'s floor (GhostmSessionSetProfile): a clade with fewer
        reads hands them to its first ancestor with min_reads. A change drops
        only the profile; the assignment under it stays."""
        m = int(min_reads)
        if not 1 <= m <= 0xFFFFFFFF:  # an int beyond uint32 would wrap
            raise GhostmError(f"profile: param: min_reads {m} outside 1..2^32 - 1")
        if native.load().GhostmSessionSetProfile(self._h, m) != 0:
            raise GhostmError(native.last_error())

    def taxon_profile(self, frame: bool = False):
        """The sample's taxon profile from read_lca(frame)'s nodes
        (GhostmSessionTaxonProfile, ...Final, ...Summary): (TAXON_COUNT_DTYPE
        records in ascending node index, one final node per read_lca record,
        the summary as a dict). Computed on first use."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionTaxonProfile(self._h, f, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        rec = np.zeros(n, dtype=TAXON_COUNT_DTYPE)
        if n and lib.GhostmSessionTaxonProfile(self._h, f, rec.ctypes.data_as(ctypes.POINTER(native.GhostmTaxonCount)), n) == bad:
            raise GhostmError(native.last_error())
        m = lib.GhostmSessionTaxonProfileFinal(self._h, f, None, 0)
        if m == bad:
            raise GhostmError(native.last_error())
        final = np.zeros(m, dtype=np.uint32)
        if m and lib.GhostmSessionTaxonProfileFinal(self._h, f, final.ctypes.data_as(_U32P), m) == bad:
            raise GhostmError(native.last_error())
        st = native.GhostmTaxonSummary()
        if lib.GhostmSessionTaxonProfileSummary(self._h, f, ctypes.byref(st), ctypes.sizeof(st)) == bad:
            raise GhostmError(native.last_error())
        return rec, final, {name: getattr(st, name) for name, _ in st._fields_}

    def taxon_profile_stats(self) -> dict:
        """The profile's counters since the last run (GhostmSessionTaxonProfileStats)."""
        st = native.GhostmTaxonProfileStats()
        native.load().GhostmSessionTaxonProfileStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def read_subject_profile(self, frame: bool, db_id: int) -> np.ndarray:
        """The 32-slot rows of subject db_id from the read-level paths, shape
        (length, 32) (GhostmSessionReadSubjectProfile): slots 27 and 28 hold
        the shift columns of a frame pile-up. Made on demand, nothing is kept."""
        lib = native.load()
        bad = ctypes.c_size_t(-1).value
        f = int(bool(frame))
        n = lib.GhostmSessionReadSubjectProfile(self._h, f, db_id, None, 0)
        if n == bad:
            raise GhostmError(native.last_error())
        prof = np.zeros(n, dtype=np.uint32)
        if n and lib.GhostmSessionReadSubjectProfile(self._h, f, db_id,
                                                     prof.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n) == bad:
            raise GhostmError(native.last_error())
        return prof.reshape(-1, 32)

    def read_pileup_stats(self) -> dict:
        """The read-level pile-up counters since the last run (GhostmSessionReadPileupStats)."""
        st = native.GhostmReadPileupStats()
        native.load().GhostmSessionReadPileupStats(self._h, ctypes.byref(st), ctypes.sizeof(st))
        return {name: getattr(st, name) for name, _ in st._fields_}

    def device_hits(self, device="cuda"):
        """The hit records as a torch uint8 tensor on this session's GPU (32 bytes
        per record, HIT_DTYPE layout), copied device-to-device — the payload of
        the multi-GPU gather."""
        import torch

        lib = native.load()
        n = lib.GhostmSessionDeviceHits(self._h, None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        out = torch.empty(max(n, 1) * HIT_DTYPE.itemsize, dtype=torch.uint8, device=device)
        if n:
            torch.cuda.synchronize(out.device)
            if lib.GhostmSessionDeviceHits(self._h, ctypes.c_void_p(out.data_ptr()), n) != n:
                raise GhostmError(native.last_error())
        return out[: n * HIT_DTYPE.itemsize]

    def device_hits_into(self, dst, cap: int) -> int:
        """Copies the hit records of the last run device-to-device into `dst` (a
        uint8 torch tensor on this session's GPU with room for `cap` records);
        returns their number. Raises if there are more than `cap`."""
        import torch

        lib = native.load()
        n = lib.GhostmSessionDeviceHits(self._h, None, 0)
        if n == ctypes.c_size_t(-1).value:
            raise GhostmError(native.last_error())
        if n > cap or dst.numel() < n * HIT_DTYPE.itemsize:
            raise GhostmError(f"{n} hit records do not fit the destination ({cap} records)")
        if n:
            torch.cuda.synchronize(dst.device)
            if lib.GhostmSessionDeviceHits(self._h, ctypes.c_void_p(dst.data_ptr()), n) != n:
                raise GhostmError(native.last_error())
        return n

    def stats(self) -> dict:
        st = native.GhostmStats()
        # the sized call: a library built with more fields writes only ours
        native.load().GhostmSessionStatsSized(self._h, ctypes.byref(st), ctypes.sizeof(st))
        out = st.as_dict()
        # the database sets' counters (GhostmSessionDbStats), under their own names
        db = native.GhostmDbSetStats()
        native.load().GhostmSessionDbStats(self._h, ctypes.byref(db), ctypes.sizeof(db))
        out.update({name: getattr(db, name) for name, _ in db._fields_})
        # the band pass's counters (GhostmSessionBandStats), likewise
        band = native.GhostmBandStats()
        native.load().GhostmSessionBandStats(self._h, ctypes.byref(band), ctypes.sizeof(band))
        out.update({name: getattr(band, name) for name, _ in band._fields_})
        return out

    def close(self) -> None:
        if self._h:
            native.load().GhostmSessionDestroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_cli(args: Sequence[str], **kw) -> subprocess.CompletedProcess:
    """Run the native `ghostm` binary (db | qry | aln | search | synth)."""
    return subprocess.run([native.BIN_PATH] + list(args), check=True, capture_output=True, **kw)


def format_db(fasta: str, prefix: str, *extra: str) -> None:
    run_cli(["db", "-i", fasta, "-o", prefix, *extra])


def format_queries(fasta: str, prefix: str, *extra: str) -> None:
    run_cli(["qry", "-i", fasta, "-o", prefix, *extra])


def synth(db_fasta: str | None, query_fasta: str | None, nq: int, db_residues: int, seed: int,
          *extra: str) -> None:
    args = ["synth", "-n", str(nq), "-N", str(db_residues), "-s", str(seed)]
    if db_fasta:
        args += ["-d", db_fasta]
    if query_fasta:
        args += ["-q", query_fasta]
    run_cli(args + list(extra))
