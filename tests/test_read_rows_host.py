"""The read-level aligned rows on the host (GhostmReadRowsHost, no device):
byte for byte against the Python model of the contract (readrows_cases.py) on
the hand-made paths and on the paths GhostmBandAlignHost / GhostmFrameAlignHost
make of every band_cases and frame_cases stage case, where the rescore proves
the DP's score and the rows spell the two sequences; every refusal with the
outputs untouched; and the host model as a stand-alone program, plain and under
-fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import band_cases as bc
import frame_cases as fc
import readrows_cases as rc
from ghostm_amd import READ_ROWS_DTYPE, native, rows_of

SRC = os.path.join(os.path.dirname(__file__), "native", "test_read_rows.cpp")


def _equal(got, want):
    assert got[0].dtype == READ_ROWS_DTYPE and got[0].itemsize == 40
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert bytes(got[1]) == bytes(want[1])


@pytest.mark.parametrize("build", [rc.hand_band_set, lambda: rc.hand_frame_set(0), lambda: rc.hand_frame_set(1)],
                         ids=["band", "frame_strand0", "frame_strand1"])
def test_hand_made_paths_equal_the_model(build):
    rs = build()
    got = rs.host()
    _equal(got, rs.model())
    rec = got[0]
    assert (rec["columns"] == [sum(int(w) >> 4 for w in bc.hit_words(rs.rec, rs.ops, h)) for h in range(len(rec))]).all()
    assert (rec["columns"] == 0).sum() == 1 and (rec["pad"] == 0).all()
    # the counts alone, one hit, no hit
    n = len(rec)
    one = rs.host(count=1)
    assert np.array_equal(one[0], rec[:1]) and bytes(one[1]) == bytes(got[1][:3 * int(rec["columns"][0])])
    none = rs.host(count=0)
    assert len(none[0]) == 0 and len(none[1]) == 0
    assert n >= 6


def test_hand_made_text():
    """What the rows say, spelled out: '?' for the codes from 25 up with the
    matrix indexed by the low five bits, and the shift columns."""
    rs = rc.hand_band_set()
    rec, rows = rs.host()
    q, m, s = rows_of(rec, rows, 4)
    assert q == b"???????" and s == b"???????" and m[0:1] == b"?" and m[2:3] == b"?"
    M = np.asarray(rs.M()).reshape(32, 32)
    want = sum(int(M[(26 + k) % 32 if k < 6 else 25, 25 + k]) for k in range(7))
    assert int(rec["rescore"][4]) == want and int(rec["identities"][4]) == 4
    q, m, s = rows_of(rec, rows, 0)
    a = bc.source_codes(rs.qseq, rs.W, rs.step, rs.src[0])
    assert q == bytes(ord(rc.LETTERS[c]) for c in a) and m == q and len(s) == 200
    fs = rc.hand_frame_set(1)
    rec, rows = fs.host()
    q, m, s = rows_of(rec, rows, 1)
    assert q[1:2] == b"/" and q[6:7] == b"\\" and m[1:2] == b" " and s[1:2] == b"-" and s[6:7] == b"-"
    assert int(rec["shifts"][1]) == 2 and int(rec["gap_residues"][1]) == 0 and int(rec["shifts"][0]) == 2
    # the '/' after the pair at strand position 30 shows letter 10 of frame 2
    frames = [bc.source_codes(fs.qseq, fs.W, fs.step, (int(fs.src["first_record"][1]) + g, 6, 3, 200)) for g in range(3)]
    assert q[0:1] == rc.LETTERS[frames[0][10]].encode() and q[2:3] == rc.LETTERS[frames[2][10]].encode()
    assert int(rec["query_record"][1]) == int(fs.src["first_record"][1])           # letter 10 of frame 0: tile 0
    assert int(rec["query_record"][2]) == int(fs.src["first_record"][2]) + 1 + 6   # position 370: letter 123 of frame 1, tile 1
    assert int(rec["query_record"][4]) == int(fs.src["first_record"][4])           # no words


def _strip(row, drop):
    return bytes(b for b in row if b not in drop)


def _check_made(rs, frames_or_sources, frame):
    got = rs.host()
    _equal(got, rs.model())
    rec, rows = got
    for h in range(len(rec)):
        words = [int(w) for w in bc.hit_words(rs.rec, rs.ops, h)]
        assert int(rec["rescore"][h]) == int(rs.rec["score"][h]), h
        assert int(rec["columns"][h]) == sum(w >> 4 for w in words)
        assert int(rec["shifts"][h]) == sum(w >> 4 for w in words if w & 15 >= 4)
        assert int(rec["gap_residues"][h]) == sum(w >> 4 for w in words if w & 15 in (2, 3))
        q, m, s = rows_of(rec, rows, h)
        # the query row spells the source from q_start on, in frame mode switching frames at the shifts
        p, want = int(rs.rec["q_start"][h]), []
        for w in words:
            for _ in range(w >> 4):
                op = w & 15
                if op <= 2:
                    c = int(frames_or_sources[h][p % 3][p // 3]) if frame else int(frames_or_sources[h][p])
                    want.append(ord(rc.letter(c)))
                    p += 3 if frame else 1
                elif op >= 4:
                    p += 1 if op == 4 else -1
        assert _strip(q, b"-/\\") == bytes(want), h
        if words:
            assert p - 1 == int(rs.rec["q_end"][h])
            lo, hi = int(rs.rec["s_start"][h]), int(rs.rec["s_end"][h])
            assert _strip(s, b"-") == bytes(ord(rc.letter(int(c))) for c in rs.db[lo:hi + 1]), h
        else:
            assert q == m == s == b""
    return rec


@pytest.mark.parametrize("name,build", bc.STAGE_CASES, ids=[n for n, _ in bc.STAGE_CASES])
def test_band_paths_rescore_and_spell_the_sequences(name, build):
    case = build()
    rec = _check_made(rc.made_band_set(case), case.sources(), False)
    assert (rec["shifts"] == 0).all()


@pytest.mark.parametrize("name,build", fc.STAGE_CASES, ids=[n for n, _ in fc.STAGE_CASES])
def test_frame_paths_rescore_and_spell_the_sequences(name, build):
    case = build()
    _check_made(rc.made_frame_set(case), case.frames(), True)


def test_planted_truth_has_one_shift():
    for kind, ch in (("ins", b"\\"), ("del", b"/")):
        rs = rc.made_frame_set(fc.truth_case(77, kind)[0])
        rec, rows = rs.host()
        q, _, _ = rows_of(rec, rows, 0)
        assert int(rec["shifts"][0]) == 1 and q.count(ch) == 1 and int(rec["rescore"][0]) == int(rs.rec["score"][0])


def _raw(lib, rs, **kw):
    """One raw GhostmReadRowsHost call into canary-filled outputs."""
    nq = kw.get("nq", rs.nq)
    qseq = np.ascontiguousarray(rs.qseq[:nq * rs.W])
    src = np.ascontiguousarray(kw.get("src", rs.src))
    rec = np.ascontiguousarray(kw.get("rec", rs.rec))
    ops = np.ascontiguousarray(kw.get("ops", rs.ops))
    M = np.ascontiguousarray(rs.M(), dtype=np.int32)
    out = np.zeros(len(src), dtype=READ_ROWS_DTYPE)
    out["columns"][:] = 0xDEADBEEF
    rows = np.full(1 << 14, 0xA7, dtype=np.uint8)
    used = ctypes.c_size_t(12345)
    rc_ = lib.GhostmReadRowsHost(
        rc._p(qseq, ctypes.c_uint8), nq, rs.W, rc._p(rs.db, ctypes.c_uint8), len(rs.db),
        M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(src),
        None if kw.get("null_src") else src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
        rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), rc._p(ops), len(ops), kw.get("W", rs.W),
        kw.get("step", rs.step), rs.frame, rs.gaps[0], rs.gaps[1], kw.get("shift", rs.shift),
        out.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)), rc._p(rows, ctypes.c_uint8),
        kw.get("rows_cap", len(rows)), ctypes.byref(used))
    untouched = (out["columns"] == 0xDEADBEEF).all() and (rows == 0xA7).all() and used.value == 12345
    return rc_, untouched


@pytest.mark.parametrize("build", [rc.hand_band_set, lambda: rc.hand_frame_set(0)], ids=["band", "frame"])
def test_refusals_leave_the_outputs_untouched(build):
    rs = build()
    lib = native.load()
    assert _raw(lib, rs) == (0, False)
    seen = set()
    for reason, kw in rc.refusal_variants(rs):
        code, untouched = _raw(lib, rs, **kw)
        assert code != 0 and native.last_error().startswith("GhostmReadRowsHost: " + reason), (reason, kw, native.last_error())
        assert untouched, (reason, kw)
        seen.add(reason)
    code, untouched = _raw(lib, rs, W=rs.W - 1)   # query_sequence_length is not the records' width
    assert code != 0 and "source" in native.last_error() and untouched
    assert seen == {"source", "ops", "word", "bounds", "rows_cap", "null"} | ({"shift"} if rs.frame else set())


def test_band_mode_reads_no_shift_cost():
    rs = rc.hand_band_set()
    lib = native.load()
    assert _raw(lib, rs, shift=7)[0] == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_model_stand_alone(flags, tmp_path):
    exe = str(tmp_path / "test_read_rows")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
