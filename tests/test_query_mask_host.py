"""The host model of the low-complexity mask (GhostmMaskRecordsHost,
ghostm_amd/csrc/query_mask_host.cpp) against the Python model of
tests/mask_cases.py: every case set (letter counts around the window and the
64-window groups, windows 6 / 12 / 32, four pairs of levels, tiled protein and
DNA layouts and an untiled one), the named carry cases, the tiles' agreement,
'*' untouched, and every refusal with its reason and the records left alone. No
device: the kernels meet the same model in test_gpu_query_mask.py."""
import numpy as np
import pytest

import mask_cases as mc
from ghostm_amd import BAND_SOURCE_DTYPE, GhostmError, mask_records_host


def check_against_model(call, records, srcs, W, step, w, levels, want, counts):
    got, masked = call(records, W, srcs, step, w, *levels)
    got = got.reshape(-1, W)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:2]], want[bad[:2]])
    assert masked.tolist() == counts.tolist()
    # '*' is never rewritten, and nothing but a letter below X is
    changed = got != records
    assert (records[changed] < mc.X).all() and (got[changed] == mc.X).all()
    assert ((records == mc.STAR) == (got == mc.STAR)).all()
    # the tiles that cover a letter agree on it
    for src in srcs:
        letters = {}
        for rec, s in mc.source_rows(src, W, step):
            for k in range(min(W, int(src["letters"]) - s)):
                assert letters.setdefault(s + k, int(got[rec, k])) == int(got[rec, k]), (src, rec, k)


def test_table_for_window_12():
    assert mc.table(12) == [0, 0, 2048, 4869, 8192, 11888, 15882, 20123, 24576, 29214, 34017, 38967, 44052]


@pytest.mark.parametrize("w,levels,layout", mc.all_case_sets())
def test_host_equals_model(w, levels, layout):
    records, srcs, step, want, counts, _ = mc.case_set(w, levels, layout)
    check_against_model(mask_records_host, records, srcs, layout[0], step, w, levels, want, counts)


@pytest.mark.parametrize("name", sorted(mc.carry_cases()))
def test_carry_cases(name):
    letters, W, step, stride, w, levels, check = mc.carry_cases()[name]
    low, trig = mc.flags(letters[0], w, *levels)
    check(low, trig, mc.mask_letters(letters[0], w, *levels))
    records, srcs = mc.lay_out(letters, W, step, stride)
    want, counts, _ = mc.model(records, srcs, W, step, w, *levels)
    check_against_model(mask_records_host, records, srcs, W, step, w, levels, want, counts)


def test_dna_frames_with_a_stop_run():
    frames = mc.dna_carry_case()
    W, step, w, levels = 40, 7, 12, (220, 250)
    records, srcs = mc.lay_out(frames, W, step, 6)
    want, counts, per_source = mc.model(records, srcs, W, step, w, *levels)
    mask = mc.mask_letters(frames[0], w, *levels)
    # frame 0: 14 Q, the stop run (TAA and the five codons up to the ATG), M, 14 Q; the stop run stays as it is
    q0 = next(i for i in range(len(frames[0])) if frames[0][i:i + 14] == [5] * 14)
    stops = list(range(q0 + 14, q0 + 20))
    assert [frames[0][i] for i in stops] == [mc.STAR] * 6 and frames[0][q0 + 21:q0 + 35] == [5] * 14
    assert all(mask[q0:q0 + 14]) and all(mask[q0 + 21:q0 + 35]) and not any(mask[i] for i in stops)
    assert sum(1 for n in per_source if n) >= 3
    check_against_model(mask_records_host, records, srcs, W, step, w, levels, want, counts)


def test_short_sources_are_left_alone():
    for w in mc.WINDOWS:
        records, srcs = mc.lay_out([[3] * (w - 1)] * 6, 20 if w < 20 else 40, 7, 6)
        got, masked = mask_records_host(records, records.shape[1], srcs, 7, w, 0, 500)
        assert got.tobytes() == records.tobytes() and not masked.any()


@pytest.mark.parametrize("reason,change", mc.REFUSALS)
def test_refusals(reason, change):
    """Four records of 20 letters, all one letter: a call that went through would mask them."""
    records, src, args = mc.refusal_args(change)
    assert src.dtype == BAND_SOURCE_DTYPE
    with pytest.raises(GhostmError, match=reason + ":"):
        mask_records_host(records, 20, src, args["step"], args["window"], args["trigger"], args["extend"])
    # in place: the library's own view of the caller's array
    import ctypes

    from ghostm_amd import native
    buf, masked = records.copy(), np.full(4, 77, dtype=np.uint32)
    rc = native.load().GhostmMaskRecordsHost(
        buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 20, len(src),
        src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)), args["step"], args["window"], args["trigger"],
        args["extend"], masked.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc != 0 and reason + ":" in native.last_error()
    assert buf.tobytes() == records.tobytes() and (masked == 77).all()


def test_null_arrays_are_refused():
    import ctypes

    from ghostm_amd import native
    lib = native.load()
    src = np.array([(0, 1, 1, 20)], dtype=BAND_SOURCE_DTYPE)
    buf, masked = np.full((1, 20), 5, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    u8, u32, sp = (buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), masked.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                   src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)))
    for a, b, c in ((None, sp, u32), (u8, None, u32), (u8, sp, None)):
        assert lib.GhostmMaskRecordsHost(a, 1, 20, 1, b, 20, 12, 220, 250, c) != 0
        assert "null:" in native.last_error()
    assert (buf == 5).all()
    # and the same call goes through: the whole record is one letter
    assert lib.GhostmMaskRecordsHost(u8, 1, 20, 1, sp, 20, 12, 220, 250, u32) == 0
    assert (buf == mc.X).all() and masked[0] == 20
