"""The frame pass's host model (GhostmFrameAlignHost, no device call): against a
Python model written from the contract on every stage shape, the checker on
every hit, the properties that tie it to the band pass, the planted truth, the
struct layouts and every refusal with the outputs untouched. The kernels
(tests/test_gpu_frame_align.py) are checked against this model."""
import ctypes

import numpy as np
import pytest

import band_cases as bc
import frame_cases as fc
from ghostm_amd import HIT_FRAME_INFO_DTYPE, HIT_PATH_DTYPE, frame_cigar, native


@pytest.mark.parametrize("name,build", fc.STAGE_CASES, ids=[n for n, _ in fc.STAGE_CASES])
def test_host_model_equals_python_model(name, build):
    case = build()
    rec, ops = case.host()
    fc.assert_equals_model(rec, ops, case.model())
    case.check(rec, ops)
    # the tile records hold the frames' letters where the contract says: frame g in records first_record + g + 6t
    for h in range(0, len(case.src), 5):
        first, stride, tiles, m = (int(x) for x in case.src[h])
        for g in range(3):
            got = bc.source_codes(case.qseq, case.W, case.step, (first + g, stride, tiles, m))
            assert np.array_equal(got, case.frames()[h][g])


@pytest.mark.parametrize("kind,B,b", fc.LANE_CASES)
def test_lane_edge_cases_equal_python_model(kind, B, b):
    case = fc.lane_edge_case(kind, B, b)
    rec, ops = case.host()
    fc.assert_equals_model(rec, ops, case.model())
    strings = case.check(rec, ops)
    inner = 0 < b < 2 * B
    # on an inner lane the planted shift is taken; on the edge lane its target is no band cell
    assert (("/" if kind == "early" else "\\") in strings[0]) == inner, strings[0]


def test_stage_cases_meet_every_edge():
    """The generator's promises: empty paths, shifts of both kinds, ranges cut on
    both sides, D negative and past the subject, sources of 1, 2 and 3 tiles."""
    strings, tiles, scores = "", set(), []
    neg = past = cut = 0
    for _, build in fc.STAGE_CASES:
        case = build()
        rec, ops = case.host()
        strings += "".join(fc.expand(fc.hit_words(rec, ops, h)) + "." for h in range(len(rec)))
        tiles |= set(int(t) for t in case.src["tiles"])
        scores += list(rec["score"])
        lo = np.array([case.ranges[k][0] for k in range(len(case.ranges))])[:len(rec)]
        neg += int((case.D.astype(np.int64) < 0).sum())
        past += int((case.D.astype(np.int64) > case.s_hi).sum())
        cut += int((case.s_lo > lo).sum())
    assert strings.count("/") >= 10 and strings.count("\\") >= 10
    assert {1, 2, 3} <= tiles
    assert sum(s == 0 for s in scores) >= 5 and sum(s > 0 for s in scores) >= 100
    assert neg >= 5 and past >= 5 and cut >= 5


PROPERTY_CASES = [c for c in fc.STAGE_CASES if c[0] in (
    "m3_B31", "m127_B1", "m128_B2_two_tiles", "m200_B2", "m203_step127_B1", "rows")]


@pytest.mark.parametrize("name,build", PROPERTY_CASES, ids=[n for n, _ in PROPERTY_CASES])
def test_properties_against_the_band_pass(name, build):
    case = build()
    band = np.stack([case.band_host(g)[0]["score"].astype(np.int64) for g in range(3)])
    # no shift affordable: the best single frame, and no shift op
    rec, ops = case.host(shift=fc.NO_SHIFT)
    assert np.array_equal(rec["score"].astype(np.int64), band.max(axis=0))
    assert ((ops & 15) < 4).all()
    case.check(rec, ops, shift=fc.NO_SHIFT)
    # non-decreasing in shift, and never below a frame's band score
    prev = rec["score"].astype(np.int64)
    for shift in (-40, -15, -6, 0):
        cur = case.host(shift=shift)[0]["score"].astype(np.int64)
        assert (cur >= prev).all(), shift
        assert (cur >= band).all(), shift
        prev = cur


@pytest.mark.parametrize("kind,op", [("ins", "\\"), ("del", "/")])
def test_planted_truth(kind, op):
    """One nucleotide inserted after codon 30 of a 60-residue stretch, or one
    deleted there: 11/1, shift -15, B = 3. One shift op of the right kind, a
    score above every single frame's, ends within two residues of the stretch's."""
    case, s0 = fc.truth_case(77, kind)
    rec, ops = case.host()
    fc.assert_equals_model(rec, ops, case.model())
    s = case.check(rec, ops)[0]
    assert s.count(op) == 1 and s.count("\\") + s.count("/") == 1, s
    single = max(int(case.band_host(g)[0]["score"][0]) for g in range(3))
    assert int(rec["score"][0]) > single > 0
    lo = int(case.s_lo[0])
    assert abs(int(rec["s_start"][0]) - (lo + s0)) <= 2 and abs(int(rec["s_end"][0]) - (lo + s0 + 59)) <= 2
    assert frame_cigar(ops).count(op) == 1


def test_record_layouts():
    assert ctypes.sizeof(native.GhostmHitFrameInfo) == 16 == HIT_FRAME_INFO_DTYPE.itemsize
    assert [n for n, _ in native.GhostmHitFrameInfo._fields_] == list(HIT_FRAME_INFO_DTYPE.names)
    assert [HIT_FRAME_INFO_DTYPE.fields[n][1] for n in HIT_FRAME_INFO_DTYPE.names] == [0, 4, 8, 12]
    assert ctypes.sizeof(native.GhostmFrameStats) == 40
    assert [n for n, _ in native.GhostmFrameStats._fields_] == [
        "seconds_frame", "frame_launches", "frame_hits", "frame_cells", "frame_dir_bytes"]


def _raw_host(case, n=None, src=None, D=None, lo=None, hi=None, W=None, step=None, B=None, gaps=None, rec=True,
              ops_cap=None, used=True, db_len=None, nq=None, shift=None):
    """GhostmFrameAlignHost with canary-filled outputs; returns (rc, rec, ops, used, error)."""
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
    rc = lib.GhostmFrameAlignHost(
        fc._p(case.qseq, ctypes.c_uint8), case.nq if nq is None else nq, case.W, fc._p(case.db, ctypes.c_uint8),
        len(case.db) if db_len is None else db_len, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), n,
        src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)), fc._p(D, ctypes.c_int32), fc._p(lo), fc._p(hi),
        case.W if W is None else W, case.step if step is None else step, case.B if B is None else B, gaps[0], gaps[1],
        case.shift if shift is None else shift,
        out.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)) if rec else None, fc._p(words),
        len(words) if ops_cap is None else ops_cap, ctypes.byref(u) if used else None)
    return rc, out, words, u.value, native.last_error()


def test_every_refusal_leaves_the_outputs_untouched():
    case = fc.mixed_case(9, 200, 31, n=12)
    rc, out, words, used, _ = _raw_host(case)
    assert rc == 0 and used > 3 and (out["score"][:-1] != 0xDEADBEEF).all() and out["score"][-1] == 0xDEADBEEF
    reasons = set()
    for reason, kw in fc.refusal_variants(case):
        rc, out, words, used, err = _raw_host(case, **kw)
        assert rc != 0 and reason in err, (reason, kw, err)
        assert (out["score"] == 0xDEADBEEF).all() and (words == 0xDEADBEEF).all() and used == 12345, (reason, kw)
        reasons.add(reason)
    assert reasons == {"source", "band", "bounds", "gaps", "ops_cap", "null", "shift"}
    assert _raw_host(case, shift=0)[0] == 0 and _raw_host(case, shift=fc.NO_SHIFT)[0] == 0
    lib = native.load()
    u = ctypes.c_size_t(7)
    assert lib.GhostmFrameAlignHost(None, 0, 0, None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, 0, 0, None, None,
                                    0, ctypes.byref(u)) == 0 and u.value == 0


def test_size_call_and_subsets():
    case = fc.mixed_case(4, 127, 31, n=12)
    all_rec, all_ops = case.host()
    rc, out, words, used, _ = _raw_host(case, rec=False)
    assert rc == 0 and used == len(all_ops)
    rc, out, words, used, _ = _raw_host(case, n=1)
    assert rc == 0 and np.array_equal(out[:1], all_rec[:1]) and np.array_equal(words[:used], all_ops[:used])
