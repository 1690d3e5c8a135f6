"""The read-level band pass's host model (GhostmBandAlignHost, no device call):
against a Python model written from the contract on every stage shape, the
checker on every hit, the issue's prototype counts, the unbanded optimum on
tiny inputs, the struct layouts and every refusal with the outputs untouched.
The kernels (tests/test_gpu_band_align.py) are checked against this model."""
import ctypes

import numpy as np
import pytest

import band_cases as bc
import tbext_cases as tx
from ghostm_amd import BAND_SOURCE_DTYPE, HIT_PATH_DTYPE, band_align_host, cigar, native


@pytest.mark.parametrize("name,build", bc.STAGE_CASES, ids=[n for n, _ in bc.STAGE_CASES])
def test_host_model_equals_python_model(name, build):
    case = build()
    rec, ops = case.host()
    bc.assert_equals_model(rec, ops, case.model())
    case.check(rec, ops)
    # the tile records hold the sources' letters where the contract says
    for h in range(0, len(case.src), 7):
        assert np.array_equal(bc.source_codes(case.qseq, case.W, case.step, case.src[h]), case.sources()[h])


def test_mixed_case_meets_every_edge():
    """The generator's promises: empty paths (the band misses the rectangle),
    bands overhanging both ends, subjects shorter than the band."""
    case = bc.mixed_case(5, 2 * bc.W + bc.STEP + 3, B=31)
    rec, ops = case.host()
    assert (rec["score"] == 0).sum() >= 5 and (rec["score"] > 0).sum() >= 30
    D, lo, hi = case.D.astype(np.int64), case.s_lo.astype(np.int64), case.s_hi.astype(np.int64)
    m = np.array([len(q) for q in case.sources()])
    assert ((D - case.B < lo) & (D + case.B >= lo)).sum() >= 5           # row 0's band overhangs s_lo
    assert ((m - 1 + D + case.B > hi) & (m - 1 + D - case.B <= hi)).sum() >= 5  # the last row's overhangs s_hi
    assert (hi - lo + 1 < 2 * case.B + 1).sum() >= 5
    assert ((D - case.B > hi) | (m - 1 + D + case.B < lo)).sum() >= 5     # misses


def test_planted_indels_are_aligned_through():
    """The issue's prototype: at B = 31 every path rescored (the checker), more
    than 127 columns and a gap run in 40 of 40; at B = 3 the model's paths, with a
    lower score where the path would leave the band."""
    case = bc.indel_case(21)
    rec, ops = case.host()
    strings = case.check(rec, ops)
    assert sum(len(s) > bc.W for s in strings) == 40
    assert sum(("I" in s) or ("D" in s) for s in strings) == 40
    rec3, ops3 = case.host(B=3)
    bc.assert_equals_model(rec3, ops3, case.model(B=3))
    case.check(rec3, ops3, B=3)
    assert (rec3["score"] <= rec["score"]).all() and (rec3["score"] < rec["score"]).any()


def test_score_equals_the_unbanded_optimum_on_tiny_inputs():
    case = bc.tiny_case(31)
    rec, ops = case.host()
    case.check(rec, ops)
    M = case.M()
    for h, q in enumerate(case.sources()):
        lo, hi = int(case.s_lo[h]), int(case.s_hi[h])
        assert int(rec["score"][h]) == bc.sw_score(q, case.db[lo:hi + 1], M), h
    assert (rec["score"] > 0).sum() >= 50


def test_hand_made_cases():
    Q = "MKVLAAGIVGLTERDQNHSCFPYW"

    def one(query, subject, d=0, B=4):
        case = bc.Case(127, 64, 1, B, [query], [subject], [(0, 0, d)])
        rec, ops = case.host()
        case.check(rec, ops)
        r = rec[0]
        return (int(r["q_start"]), int(r["q_end"]), int(r["s_start"]), int(r["s_end"])), cigar(ops)

    assert one(Q, Q) == ((0, 23, 1, 24), "24=")
    assert one(Q, Q[:12] + "WW" + Q[12:]) == ((0, 23, 1, 26), "12=2D12=")
    assert one(Q, Q[:12] + Q[14:]) == ((0, 23, 1, 22), "12=2I10=")
    assert one(Q, Q[:12] + "WW" + Q[12:], B=1) == ((0, 11, 1, 12), "12=")   # the gap of two leaves a band of one
    assert one(Q, "WWWWW" + Q, d=5) == ((0, 23, 6, 29), "24=")
    assert one(Q, Q, d=40) == ((0, 0, 1, 1), "")                           # the band misses the subject


def test_record_layouts():
    assert ctypes.sizeof(native.GhostmBandSource) == 16 == BAND_SOURCE_DTYPE.itemsize
    assert [n for n, _ in native.GhostmBandSource._fields_] == list(BAND_SOURCE_DTYPE.names)
    assert [BAND_SOURCE_DTYPE.fields[n][1] for n in BAND_SOURCE_DTYPE.names] == [
        getattr(native.GhostmBandSource, n).offset for n in BAND_SOURCE_DTYPE.names] == [0, 4, 8, 12]
    assert ctypes.sizeof(native.GhostmBandStats) == 40
    assert [n for n, _ in native.GhostmBandStats._fields_] == [
        "seconds_band", "band_launches", "band_hits", "band_cells", "band_dir_bytes"]


def _raw_host(case, n=None, src=None, D=None, lo=None, hi=None, W=None, step=None, B=None, gaps=None, rec=True,
              ops_cap=None, used=True, db_len=None, nq=None):
    """GhostmBandAlignHost with canary-filled outputs; returns (rc, rec, ops, used, error)."""
    lib = native.load()
    n = len(case.src) if n is None else n
    src = np.ascontiguousarray(case.src if src is None else src)
    D = np.ascontiguousarray(case.D if D is None else D, dtype=np.int32)
    lo = np.ascontiguousarray(case.s_lo if lo is None else lo, dtype=np.uint32)
    hi = np.ascontiguousarray(case.s_hi if hi is None else hi, dtype=np.uint32)
    M = np.ascontiguousarray(case.M(), dtype=np.int32)
    gaps = case.gaps if gaps is None else gaps
    out = np.zeros(n + 1, dtype=HIT_PATH_DTYPE)
    out["score"][:] = 0xDEADBEEF
    words = np.full(4096, 0xDEADBEEF, dtype=np.uint32)
    u = ctypes.c_size_t(12345)
    rc = lib.GhostmBandAlignHost(
        bc._p(case.qseq, ctypes.c_uint8), case.nq if nq is None else nq, case.W, bc._p(case.db, ctypes.c_uint8),
        len(case.db) if db_len is None else db_len, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n,
        src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)), bc._p(D, ctypes.c_int32), bc._p(lo), bc._p(hi),
        case.W if W is None else W, case.step if step is None else step, case.B if B is None else B, gaps[0], gaps[1],
        out.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)) if rec else None, bc._p(words),
        len(words) if ops_cap is None else ops_cap, ctypes.byref(u) if used else None)
    return rc, out, words, u.value, native.last_error()


def test_every_refusal_leaves_the_outputs_untouched():
    case = bc.mixed_case(5, 2 * bc.W + bc.STEP + 3, B=31, n=12)
    rc, out, words, used, _ = _raw_host(case)
    assert rc == 0 and used > 3 and (out["score"][:-1] != 0xDEADBEEF).all() and out["score"][-1] == 0xDEADBEEF
    for reason, kw in bc.refusal_variants(case):
        rc, out, words, used, err = _raw_host(case, **kw)
        assert rc != 0 and reason in err, (reason, kw, err)
        assert (out["score"] == 0xDEADBEEF).all() and (words == 0xDEADBEEF).all() and used == 12345, (reason, kw)
    lib = native.load()
    u = ctypes.c_size_t(7)
    assert lib.GhostmBandAlignHost(None, 0, 0, None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, 0, None, None, 0,
                                   ctypes.byref(u)) == 0 and u.value == 0
    assert lib.GhostmBandAlignHost(bc._p(case.qseq, ctypes.c_uint8), case.nq, case.W, bc._p(case.db, ctypes.c_uint8),
                                   len(case.db), None, 1, None, None, None, None, case.W, case.step, 31, -11, -1, None,
                                   None, 0, ctypes.byref(u)) != 0 and "null" in native.last_error()


def test_size_call_and_subsets():
    case = bc.mixed_case(3, bc.W, B=31, n=12)
    all_rec, all_ops = case.host()
    rc, out, words, used, _ = _raw_host(case, rec=False)
    assert rc == 0 and used == len(all_ops)
    one = band_align_host(case.qseq, case.W, case.db, tx.blosum62(), case.src[:1], case.D[:1], case.s_lo[:1],
                          case.s_hi[:1], case.step, case.B)
    assert np.array_equal(one[0], all_rec[:1]) and np.array_equal(one[1], all_ops[:len(one[1])])
