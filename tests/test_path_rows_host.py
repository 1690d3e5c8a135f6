"""The aligned residue rows' host model (GhostmPathRowsHost, no device call):
against a Python model written from the contract, byte for byte; the
invariants on every hit of the indel fixture; hand-made paths no traceback
would produce; the refused calls. The kernel (tests/test_gpu_path_rows.py) is
checked against this model."""
import ctypes

import numpy as np
import pytest

import pathrows_cases as pr
import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import HIT_ROWS_DTYPE, native, path_rows_host, rows_of

CASES = [
    (24, "blosum62", (-11, -1)),
    (75, "blosum62", (-11, -1)),
    (24, "pam250", (-14, -2)),
    (75, "pam250", (-14, -2)),
]


@pytest.fixture(scope="module", params=CASES, ids=["L24", "L75", "L24_pam250_g14e2", "L75_pam250_g14e2"])
def fixture_run(request, data_root):
    """The fixture's chunk, the host model's paths of its 60 hits and their rows."""
    L, matrix, gaps = request.param
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, L, matrix, gaps)
    out, rows = pr.rows_via(pr.host_call(native.load(), chunk, M, *gaps), qid, rec, ops)
    return L, chunk, M, gaps, qid, rec, ops, out, rows


def test_record_layout():
    assert ctypes.sizeof(native.GhostmHitRows) == 32 == HIT_ROWS_DTYPE.itemsize
    assert [n for n, _ in native.GhostmHitRows._fields_] == list(HIT_ROWS_DTYPE.names)
    assert [HIT_ROWS_DTYPE.fields[n][1] for n in HIT_ROWS_DTYPE.names] == [
        getattr(native.GhostmHitRows, n).offset for n in HIT_ROWS_DTYPE.names]
    assert HIT_ROWS_DTYPE["rescore"] == np.dtype("<i4")


def test_host_model_equals_python_model(fixture_run):
    L, (nq, L_, qseq, dbseq, pos), M, gaps, qid, rec, ops, out, rows = fixture_run
    assert len(qid) == 60
    pr.assert_equals_model(qseq, L, dbseq, M, qid, rec, ops, out, rows, *gaps)
    # the wrapper gives the same
    w_out, w_rows = path_rows_host(qseq, L, dbseq, M, qid, rec, ops, *gaps)
    assert np.array_equal(w_out, out) and np.array_equal(w_rows, rows)


def _kinds(fixture_run):
    L, (nq, L_, qseq, dbseq, pos), M, gaps, qid, rec, ops, out, rows = fixture_run
    kinds = set()
    for h in range(len(qid)):
        q = int(qid[h])
        kinds |= pr.check_rows(qseq[q * L:(q + 1) * L], dbseq, M, rec[h], tp.hit_words(rec, ops, h), out[h],
                               *rows_of(out, rows, h))
    return kinds


def test_invariants_on_all_hits(fixture_run):
    _kinds(fixture_run)


def test_fixture_covers_every_midline_and_gap_kind(fixture_run):
    """Letter, '+' and space in the midline, I and D columns: all occur."""
    assert _kinds(fixture_run) == pr.ALL_KINDS
    L, chunk, M, gaps, qid, rec, ops, out, rows = fixture_run
    assert int((out["gap_residues"] > 0).sum()) >= 20
    assert (out["positives"] >= out["identities"]).all()  # no identical pair of these 20 residues scores <= 0


def test_hand_made_paths(data_root):
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    assert nq == 24 and L == 127 and 300 <= len(dbseq) < 1000
    M = tx.blosum62()
    qid, rec, ops = pr.hand_paths(nq, L, len(dbseq))
    out, rows = pr.rows_via(pr.host_call(native.load(), chunk, M), qid, rec, ops)
    assert out["columns"].tolist() == pr.HAND_COLUMNS
    pr.assert_equals_model(qseq, L, dbseq, M, qid, rec, ops, out, rows, -11, -1)
    # an empty path: no bytes, no counts
    assert tuple(out[0])[1:6] == (0, 0, 0, 0, 0) and rows_of(out, rows, 0) == (b"", b"", b"")
    # gaps only: every column a gap, open once per word
    assert out["gap_residues"][13] == 197 and out["rescore"][13] == -11 - 69 - 11 - 126
    q, mid, s = rows_of(out, rows, 13)
    assert q[:70] == b"-" * 70 and s[70:] == b"-" * 127 and mid == b" " * 197
    # two I words in a row open twice
    assert out["rescore"][11] - sum(int(M[int(dbseq[200 + k]) * 32 + int(qseq[(nq - 1) * L + 91 + k])])
                                    for k in range(30)) == -11 - 1 - 11 - 2 - 11 - 3 - 11
    # the rare letters, the END code and the gap and midline signs all occur
    letters = set(bytes(rows).decode())
    assert {"B", "Z", "X", "*", "?", "-", "+", " "} <= letters


def test_identical_pair_without_score_is_not_a_positive():
    """X/X scores -1 in BLOSUM62: a '=' column, the letter in the midline, an
    identity, but no positive."""
    from ghostm_amd import HIT_PATH_DTYPE

    M = tx.blosum62()
    X = pr.LETTERS.index("X")
    assert M[X * 32 + X] <= 0
    q = np.array([0, X, 1], dtype=np.uint8)
    db = np.array([tx.END, 0, X, 1, tx.END], dtype=np.uint8)
    rec = np.zeros(1, dtype=HIT_PATH_DTYPE)
    rec[0] = (0, 2, 1, 3, 0, 1, 0)
    out, rows = path_rows_host(q, 3, db, M, [0], rec, [3 << 4])
    assert rows_of(out, rows, 0) == (b"AXR", b"AXR", b"AXR")
    assert (out["identities"][0], out["positives"][0]) == (3, 2)
    assert out["rescore"][0] == M[0] + M[X * 32 + X] + M[1 * 32 + 1]


def test_no_hits():
    lib = native.load()
    used = ctypes.c_size_t(7)
    assert lib.GhostmPathRowsHost(None, 0, 0, None, 0, None, 0, None, None, None, 0, 0, 0, 0, None, None, 0,
                                  ctypes.byref(used)) == 0
    assert used.value == 0


def test_refusals(data_root):
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    pr.check_refusals(pr.host_call(native.load(), chunk, tx.blosum62()), nq, L, len(dbseq))
