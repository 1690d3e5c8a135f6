"""The numpy model of K2 and K3 (dp_cases.py) against the oracle's per-candidate
and per-traceback dumps at every fixture width, and the conditions that keep
the GPU comparison with that model (test_gpu_dp_edges.py) from passing
vacuously. No device here."""
import os

import numpy as np
import pytest

import cases
import dp_cases as dp
import tbext_cases as tx

BLOSUM62_FILE = os.path.join(cases.GOLDEN, "matrices", "BLOSUM62")
ORACLE_RUNS = [
    ("blosum62", (-11, -1), ["-M", BLOSUM62_FILE]),
    ("blosum62", (-8, -1), ["-M", BLOSUM62_FILE, "-G", "8", "-E", "1"]),
    ("pam250", (-11, -1), ["-M", cases.PAM250]),
    ("pam250", (-8, -1), ["-M", cases.PAM250, "-G", "8", "-E", "1"]),
]


def test_layout_table():
    """The (S, G) table the widths were chosen from is what ChooseLayout's rule
    gives at the score window and at both traceback windows, and the widths are
    both ends of every range."""
    for L in range(1, 128):
        want = dp.expected_layout(L)
        for width in (dp.score_base(L), dp.trace_base(L), dp.trace_base(L, region=64)):
            assert dp.choose_layout(L, width) == want, (L, width)
    assert sorted(dp.WIDTHS) == sorted({x for lo_hi in dp.LAYOUTS for x in lo_hi})
    assert len(set(dp.LAYOUTS.values())) == 13
    assert dp.expected_layout(100) == (16, 7) and dp.expected_layout(40) == (8, 5)


@pytest.mark.parametrize("L", dp.K2_WIDTHS)
def test_model_equals_oracle(L, data_root):
    fx = dp.fixture(data_root, L)
    for mname, gaps, opts in ORACLE_RUNS:
        cand, tb = fx.oracle(opts, f"{mname}_g{-gaps[0]}e{-gaps[1]}")
        assert np.array_equal(cand[:, :2], np.stack(fx.candidates(), axis=1))  # K1 does not depend on the matrix
        M = dp.matrix(mname)
        score, end = dp.score_model(fx.qseq, L, fx.db, M, cand[:, 0], cand[:, 1], dp.score_base(L), 2, *gaps)
        assert np.array_equal(score, cand[:, 2]), (mname, gaps)
        assert np.array_equal(end, cand[:, 3]), (mname, gaps)
        assert len(tb) >= 30
        start, alen, match = dp.trace_model(fx.qseq, L, fx.db, M, tb[:, 0], tb[:, 1], dp.trace_base(L), *gaps)
        assert np.array_equal(start, tb[:, 2]), (mname, gaps)
        assert np.array_equal(alen, tb[:, 3]), (mname, gaps)
        assert np.array_equal(match, tb[:, 4]), (mname, gaps)


@pytest.mark.parametrize("L", [1, 9, 40])
def test_trace_model_equals_the_per_hit_model(L, data_root):
    """The hand-placed hits (the only ones at L = 1, which does not seed) against
    the one-hit Python model of the extended traceback, at both windows."""
    fx = dp.fixture(data_root, L)
    qid, end = dp.hand_hits(fx)
    assert (end < dp.trace_base(L)).any() and int(end.max()) == len(fx.db) - 2
    assert (np.bincount(qid) % 2 == 1).any()
    for mname, gaps in (("blosum62", (-11, -1)), ("diag11", (-11, -1)), ("pam250", (-8, -1))):
        M = dp.matrix(mname)
        for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
            start, alen, match = dp.trace_model(fx.qseq, L, fx.db, M, qid, end, base, *gaps)
            for i in range(len(qid)):
                r = tx.py_model(fx.qseq[qid[i] * L:(qid[i] + 1) * L], fx.db, M, int(end[i]), base, *gaps)
                assert (r["start"], r["len"], r["match"]) == (start[i], alen[i], match[i]), (mname, base, i)


@pytest.mark.parametrize("L", dp.K2_WIDTHS)
def test_fixture_is_not_vacuous(L, data_root):
    fx = dp.fixture(data_root, L)
    qid, start = fx.candidates()
    assert len(qid) >= 200
    per_query = np.bincount(qid, minlength=fx.nq)
    classes = np.array(fx.classes)
    for c in sorted(set(fx.classes)):
        assert per_query[classes == c].sum() >= 1, c
    # queries that draw 1, 2, 3 and >= 24 candidates
    for want in (1, 2, 3):
        assert per_query[fx.classes.index(f"cands{want}")] == want
    assert (per_query[classes == "cands24"] >= 24).all()
    M = dp.matrix("diag11")
    score, end, det = dp.score_model(fx.qseq, L, fx.db, M, qid, start, dp.score_base(L), 2, -11, -1, detail=True)
    assert np.array_equal(score, dp.model_scores(data_root, L, "diag11")[0])
    assert (det["ties"] > 0).any()          # an end-column tie: >= decides the end
    assert (det["ends"] >= 2).any()         # a window with two or more ENDs
    assert (det["ends"] == 1).any() and (det["ends"] >= 4).any()
    assert det["clipped_lo"].any() and det["clipped_hi"].any()
    # an exact copy scores exactly L * m
    scales = dp.SCALES if L in dp.SWEEP_WIDTHS else [11]
    exact = np.isin(qid, [i for i, c in enumerate(fx.classes) if c.startswith("exact")])
    assert len(set(qid[exact].tolist())) == 8
    for m in scales:
        score, _ = dp.score_model(fx.qseq, L, fx.db, dp.matrix(f"diag{m}"), qid[exact], start[exact], dp.score_base(L),
                                  2, -11, -1)
        for i in set(qid[exact].tolist()):
            assert score[qid[exact] == i].max() == L * m, (m, i)
    # the all-negative and the all-zero matrix: score 0, end = the window's last residue column
    for mname in ("neg", "zero"):
        score, end = dp.model_scores(data_root, L, mname)
        assert not score.any()
        off = np.maximum(start.astype(np.int64) - 2, 0)
        for i in range(0, len(qid), 7):
            w = fx.db[off[i]:off[i] + dp.score_base(L)]
            assert end[i] == off[i] + np.flatnonzero(w != dp.END).max()


@pytest.mark.parametrize("L", [100])
def test_sweep_width_100(L, data_root):
    """The S = 16 sweep width is no layout-range end: its fixture is checked like the others."""
    test_model_equals_oracle(L, data_root)
    test_fixture_is_not_vacuous(L, data_root)


@pytest.mark.parametrize("L", dp.SWEEP_WIDTHS)
def test_db_codes_variant_is_not_vacuous(L, data_root):
    """The DB patched to the codes 26..31: the model's scores move, and they
    differ from both readings a kernel could wrongly make of such a code (a
    zero matrix row; an END), so the GPU comparison tells them apart."""
    fx = dp.fixture(data_root, L)
    qid, start = fx.candidates()
    db = fx.db_codes()
    assert sorted(set(db[db > dp.END].tolist())) == [26, 27, 28, 29, 30, 31] and int((db > dp.END).sum()) == 24
    assert np.array_equal(db == dp.END, fx.db == dp.END)
    M = dp.matrix("diag11x")
    assert int(np.abs(M).max()) == 11 and M.reshape(32, 32)[26:, :25].all()
    plain = dp.model_scores(data_root, L, "diag11")
    want = dp.model_scores(data_root, L, "diag11x", codes=True)
    Mz = M.reshape(32, 32).copy()
    Mz[25:] = 0
    zero_rows = dp.score_model(fx.qseq, L, db, Mz.reshape(-1), qid, start, dp.score_base(L), 2, -11, -1)
    as_end = dp.score_model(fx.qseq, L, np.where(db > dp.END, dp.END, db), M, qid, start, dp.score_base(L), 2, -11, -1)
    for other in (plain, zero_rows, as_end):
        assert int((other[0] != want[0]).sum()) >= 10
    (hq, he), tr = dp.model_traces(data_root, L, "diag11x", codes=True)
    tz = dp.trace_model(fx.qseq, L, db, Mz.reshape(-1), hq, he, dp.trace_base(L), -11, -1)
    assert int(((tz[0] != tr[0]) | (tz[1] != tr[1])).sum()) >= 5
