"""The extended traceback's host model (GhostmTraceBackExtHost, no device call):
against a Python model written from the contract, against the oracle's
traceback, on hand-made cases with known answers, and its invariants. The
kernel (tests/test_gpu_traceback_ext.py) is checked against this model."""
import ctypes

import numpy as np
import pytest

import tbext_cases as tx
from ghostm_amd import HIT_EXT_DTYPE, native, traceback_ext_host


def _base(L, log_region=4, extend=2):
    return L + 2 * extend * 2 * (1 << log_region)


@pytest.fixture(scope="module", params=[24, 75])
def fixture_run(request, data_root):
    """Fixture at L, the oracle's 60 hits, and the host model's results on them."""
    L = request.param
    d, (nq, L_, qseq, dbseq, pos), tb = tx.fixture_hits(data_root, L)
    assert L_ == L and nq == 60
    out = traceback_ext_host(qseq, L, dbseq, tx.blosum62(), tb[:, 0], tb[:, 1], _base(L))
    tx.assert_gapped(out[1], out[2], out[3])
    return L, qseq, dbseq, tb, out


def test_python_model_equals_host_model(fixture_run):
    L, qseq, dbseq, tb, (start, alen, match, ext) = fixture_run
    M = tx.blosum62()
    dels = []
    for h in range(len(tb)):
        q = int(tb[h, 0])
        r = tx.py_model(qseq[q * L:(q + 1) * L], dbseq, M, int(tb[h, 1]), _base(L))
        got = (int(start[h]), int(alen[h]), int(match[h]), int(ext["q_start"][h]), int(ext["q_end"][h]),
               int(ext["mismatches"][h]), int(ext["gap_opens"][h]))
        want = (r["start"], r["len"], r["match"], r["q_start"], r["q_end"], r["mism"], r["gapopen"])
        assert got == want, (h, got, want)
        dels.append(r["dels"])
    tx.check_invariants(alen, match, ext, dels)


def test_host_model_equals_oracle_traceback(fixture_run):
    """(db_start, aln_len, aln_match) are the reference's (the oracle's .tb dump)."""
    L, qseq, dbseq, tb, (start, alen, match, ext) = fixture_run
    assert np.array_equal(start, tb[:, 2])
    assert np.array_equal(alen, tb[:, 3])
    assert np.array_equal(match, tb[:, 4])


def test_invariants_on_all_hits(fixture_run):
    L, qseq, dbseq, tb, (start, alen, match, ext) = fixture_run
    tx.check_invariants(alen, match, ext)
    assert (ext["q_end"] < L).all() and (ext["q_start"] <= ext["q_end"]).all()


# ------------------------------------------------------- hand-made cases
Q24 = "MKVLAAGIVGLTERDQNHSCFPYW"  # no residue twice in a row


def _one(query, db_codes, end=None):
    q = tx.codes(query)
    L = len(q)
    db = np.array(db_codes, dtype=np.uint8)
    end = len(db) - 2 if end is None else end  # the last residue before the closing END
    start, alen, match, ext = traceback_ext_host(q, L, db, tx.blosum62(), [0], [end], _base(L))
    r = tx.py_model(q, db, tx.blosum62(), end, _base(L))
    assert (r["start"], r["len"], r["match"], r["q_start"], r["q_end"], r["mism"], r["gapopen"]) == (
        int(start[0]), int(alen[0]), int(match[0]), int(ext["q_start"][0]), int(ext["q_end"][0]),
        int(ext["mismatches"][0]), int(ext["gap_opens"][0]))
    return int(start[0]), int(alen[0]), int(match[0]), tuple(int(ext[f][0]) for f in
                                                             ("q_start", "q_end", "mismatches", "gap_opens"))


def test_exact_copy():
    q = list(tx.codes(Q24))
    start, alen, match, ext = _one(Q24, [tx.END] + q + [tx.END])
    assert (start, alen, match) == (1, 24, 24)
    assert ext == (0, 23, 0, 0)


def test_one_substitution():
    q = list(tx.codes(Q24))
    q[12] = tx.AA.index("W")  # E -> W scores -3
    start, alen, match, ext = _one(Q24, [tx.END] + q + [tx.END])
    assert (start, alen, match) == (1, 24, 23)
    assert ext == (0, 23, 1, 0)


def test_two_residue_gap_in_the_query():
    q = list(tx.codes(Q24))
    w = tx.AA.index("W")
    start, alen, match, ext = _one(Q24, [tx.END] + q[:12] + [w, w] + q[12:] + [tx.END])
    assert (start, alen, match) == (1, 26, 24)  # 24 matches, 2 gap residues
    assert ext == (0, 23, 0, 1)


def test_two_residue_gap_in_the_subject():
    q = list(tx.codes(Q24))
    start, alen, match, ext = _one(Q24, [tx.END] + q[:12] + q[14:] + [tx.END])
    assert (start, alen, match) == (1, 24, 22)  # 22 matches, 2 gap residues
    assert ext == (0, 23, 0, 1)


def test_window_cut_by_end():
    q = list(tx.codes(Q24))
    start, alen, match, ext = _one(Q24, [tx.END] + q[:10] + [tx.END] + q[10:] + [tx.END])
    assert (start, alen, match) == (12, 14, 14)
    assert ext == (10, 23, 0, 0)


def test_window_clipped_at_db_position_zero():
    q = list(tx.codes(Q24))
    start, alen, match, ext = _one(Q24, q + [tx.END], end=23)
    assert (start, alen, match) == (0, 24, 24)
    assert ext == (0, 23, 0, 0)


def test_no_hits_and_bad_hits():
    lib = native.load()
    assert lib.GhostmTraceBackExtHost(None, 0, 0, None, 0, None, 0, None, None, 0, 0, 0, None, None, None, None) == 0
    q = tx.codes(Q24)
    with pytest.raises(Exception):
        traceback_ext_host(q, 24, np.array([tx.END], dtype=np.uint8), tx.blosum62(), [1], [0], _base(24))


def test_record_layout():
    assert ctypes.sizeof(native.GhostmHitExt) == 16 == HIT_EXT_DTYPE.itemsize
    assert [n for n, _ in native.GhostmHitExt._fields_] == list(HIT_EXT_DTYPE.names)
