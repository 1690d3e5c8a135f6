"""The alignment path's host model (GhostmTraceBackPathHost, no device call):
against a Python model written from the contract, its invariants (every path
re-walked along the two sequences), hand-made cases, the empty and the
refused calls. The kernels (tests/test_gpu_traceback_path.py) are checked
against this model."""
import ctypes

import numpy as np
import pytest

import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import HIT_PATH_DTYPE, cigar, native, traceback_ext_host, traceback_path_host


def _base(L, log_region=4, extend=2):
    return L + 2 * extend * 2 * (1 << log_region)


CASES = [
    (24, (), "blosum62", (-11, -1)),
    (75, (), "blosum62", (-11, -1)),
    (24, ("-M", tx.cases.PAM250, "-G", "14", "-E", "2"), "pam250", (-14, -2)),
    (75, ("-M", tx.cases.PAM250, "-G", "14", "-E", "2"), "pam250", (-14, -2)),
]


@pytest.fixture(scope="module", params=CASES, ids=["L24", "L75", "L24_pam250_g14e2", "L75_pam250_g14e2"])
def fixture_run(request, data_root):
    """Fixture at L, the oracle's 60 hits, the extended host model's records and
    the path host model's results with and without the known starts."""
    L, opts, matrix, gaps = request.param
    d, (nq, L_, qseq, dbseq, pos), tb = tx.fixture_hits(data_root, L, opts)
    assert L_ == L and nq == 60
    M = tx.blosum62() if matrix == "blosum62" else tx.pam250()
    ext = traceback_ext_host(qseq, L, dbseq, M, tb[:, 0], tb[:, 1], _base(L), *gaps)
    free = traceback_path_host(qseq, L, dbseq, M, tb[:, 0], tb[:, 1], _base(L), *gaps)
    known = traceback_path_host(qseq, L, dbseq, M, tb[:, 0], tb[:, 1], _base(L), *gaps, db_starts_in=tb[:, 2])
    return L, qseq, dbseq, tb, M, gaps, ext, free, known


def test_known_starts_change_nothing(fixture_run):
    L, qseq, dbseq, tb, M, gaps, ext, free, known = fixture_run
    assert np.array_equal(free[0], known[0]) and np.array_equal(free[1], known[1])


def test_python_model_equals_host_model(fixture_run):
    L, qseq, dbseq, tb, M, gaps, ext, (rec, ops), known = fixture_run
    for h in range(len(tb)):
        q, end = int(tb[h, 0]), int(tb[h, 1])
        for max_cols in (None, end - int(tb[h, 2]) + 1):
            r = tp.path_model(qseq[q * L:(q + 1) * L], dbseq, M, end, _base(L), gaps[0], gaps[1], max_cols)
            got = tuple(int(rec[f][h]) for f in ("q_start", "q_end", "s_start", "s_end", "score"))
            assert got == (r["q_start"], r["q_end"], r["s_start"], r["s_end"], r["score"]), (h, got, r)
            assert list(tp.hit_words(rec, ops, h)) == tp.runs(r["ops"]), (h, r["ops"])
    assert np.array_equal(rec["ops_offset"], np.concatenate([[0], np.cumsum(rec["n_runs"])[:-1]]))
    assert len(ops) == int(rec["n_runs"].sum())


def test_invariants_on_all_hits(fixture_run):
    L, qseq, dbseq, tb, M, gaps, (e_start, e_len, e_match, e_ext), (rec, ops), known = fixture_run
    for h in range(len(tb)):
        q = int(tb[h, 0])
        tp.check_path(qseq[q * L:(q + 1) * L], dbseq, M, rec[h], tp.hit_words(rec, ops, h), gaps[0], gaps[1],
                      db_start=tb[h, 2], ext=tuple(e_ext[h]), aln=(e_len[h], e_match[h]))
    assert (rec["q_end"] < L).all() and (rec["s_end"] <= tb[:, 1]).all()


def test_the_fixture_has_gaps(fixture_run):
    L, qseq, dbseq, tb, M, gaps, ext, (rec, ops), known = fixture_run
    if gaps == (-11, -1):
        tp.assert_gapped(rec, ops)


# ------------------------------------------------------- hand-made cases
Q24 = "MKVLAAGIVGLTERDQNHSCFPYW"  # no residue twice in a row


def _one(query, db_codes, end=None):
    q = tx.codes(query)
    L = len(q)
    db = np.array(db_codes, dtype=np.uint8)
    end = len(db) - 2 if end is None else end  # the last residue before the closing END
    rec, ops = traceback_path_host(q, L, db, tx.blosum62(), [0], [end], _base(L))
    r = tp.path_model(q, db, tx.blosum62(), end, _base(L))
    assert list(ops) == tp.runs(r["ops"])
    tp.check_path(q, db, tx.blosum62(), rec[0], ops, -11, -1)
    return tuple(int(rec[f][0]) for f in ("q_start", "q_end", "s_start", "s_end")), cigar(ops)


def test_exact_copy():
    q = list(tx.codes(Q24))
    assert _one(Q24, [tx.END] + q + [tx.END]) == ((0, 23, 1, 24), "24=")


def test_one_substitution():
    q = list(tx.codes(Q24))
    q[12] = tx.AA.index("W")  # E -> W scores -3
    assert _one(Q24, [tx.END] + q + [tx.END]) == ((0, 23, 1, 24), "12=1X11=")


def test_two_residue_gap_in_the_query():
    q = list(tx.codes(Q24))
    w = tx.AA.index("W")
    assert _one(Q24, [tx.END] + q[:12] + [w, w] + q[12:] + [tx.END]) == ((0, 23, 1, 26), "12=2D12=")


def test_two_residue_gap_in_the_subject():
    q = list(tx.codes(Q24))
    assert _one(Q24, [tx.END] + q[:12] + q[14:] + [tx.END]) == ((0, 23, 1, 22), "12=2I10=")


def test_window_cut_by_end():
    q = list(tx.codes(Q24))
    assert _one(Q24, [tx.END] + q[:10] + [tx.END] + q[10:] + [tx.END]) == ((10, 23, 12, 25), "14=")


def test_window_clipped_at_db_position_zero():
    q = list(tx.codes(Q24))
    assert _one(Q24, q + [tx.END], end=23) == ((0, 23, 0, 23), "24=")


def test_path_may_end_before_the_hit_end():
    """The reverse DP's maximum lies where the forward alignment began; residues
    behind the alignment that score below zero are not part of the path."""
    q = list(tx.codes(Q24))
    w = tx.AA.index("W")
    got = _one(Q24[:20] + "AAAA", [tx.END] + q[:20] + [w, w, w, w] + [tx.END])
    assert got == ((0, 19, 1, 20), "20=")


def test_cigar():
    assert cigar([31 << 4 | 0, 1 << 4 | 1, 2 << 4 | 3, 40 << 4 | 0]) == "31=1X2D40="
    assert cigar([3 << 4 | 2]) == "3I" and cigar([]) == ""


# ------------------------------------------------------- sizes, empty and refused calls
def test_record_layout():
    assert ctypes.sizeof(native.GhostmHitPath) == 32 == HIT_PATH_DTYPE.itemsize
    assert [n for n, _ in native.GhostmHitPath._fields_] == list(HIT_PATH_DTYPE.names)
    assert [HIT_PATH_DTYPE.fields[n][1] for n in HIT_PATH_DTYPE.names] == [
        getattr(native.GhostmHitPath, n).offset for n in HIT_PATH_DTYPE.names]


def test_no_hits_and_one_hit(data_root):
    lib = native.load()
    used = ctypes.c_size_t(7)
    assert lib.GhostmTraceBackPathHost(None, 0, 0, None, 0, None, 0, None, None, None, 0, 0, 0, None, None, 0,
                                       ctypes.byref(used)) == 0
    assert used.value == 0
    d, (nq, L, qseq, dbseq, pos), tb = tx.fixture_hits(data_root, 24)
    M = tx.blosum62()
    rec, ops = traceback_path_host(qseq, L, dbseq, M, tb[:0, 0], tb[:0, 1], _base(L))
    assert len(rec) == 0 and len(ops) == 0
    all_rec, all_ops = traceback_path_host(qseq, L, dbseq, M, tb[:, 0], tb[:, 1], _base(L))
    rec, ops = traceback_path_host(qseq, L, dbseq, M, tb[:1, 0], tb[:1, 1], _base(L))
    assert np.array_equal(rec, all_rec[:1]) and np.array_equal(ops, all_ops[:len(ops)]) and len(ops) == rec["n_runs"][0]


def test_refusals(data_root):
    d, (nq, L, qseq, dbseq, pos), tb = tx.fixture_hits(data_root, 24)
    M = tx.blosum62()
    lib = native.load()
    with pytest.raises(Exception, match="outside"):
        traceback_path_host(qseq, L, dbseq, M, [nq], [tb[0, 1]], _base(L))
    with pytest.raises(Exception, match="outside"):
        traceback_path_host(qseq, L, dbseq, M, [0], [len(dbseq)], _base(L))
    with pytest.raises(Exception, match="start after end"):
        traceback_path_host(qseq, L, dbseq, M, [0], [tb[0, 1]], _base(L), db_starts_in=[tb[0, 1] + 1])
    with pytest.raises(Exception, match="window"):
        traceback_path_host(qseq, L, dbseq, M, tb[:1, 0], tb[:1, 1], 32768 - L)
    q128 = np.zeros(128, dtype=np.uint8)
    with pytest.raises(Exception, match="127"):
        traceback_path_host(q128, 128, dbseq, M, [0], [tb[0, 1]], 200)
    # a buffer too small for the words is an error, and nothing is written past it
    qid, end = np.ascontiguousarray(tb[:, 0]), np.ascontiguousarray(tb[:, 1])
    Mi = np.ascontiguousarray(M, dtype=np.int32)
    ops = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    used = ctypes.c_size_t(0)
    rc = lib.GhostmTraceBackPathHost(tx._p(qseq, ctypes.c_uint8), nq, L, tx._p(dbseq, ctypes.c_uint8), len(dbseq),
                                     Mi.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(qid), tx._p(qid),
                                     tx._p(end), None, _base(L), -11, -1, None, tx._p(ops), 4, ctypes.byref(used))
    assert rc != 0 and "ops_cap" in native.last_error()
    assert (ops[4:] == 0xDEADBEEF).all()
