"""K1's candidates, K2's (score, end) and K3's (start, len, match) through the
reference plugin ABI against the numpy model of dp_cases.py: at both ends of
every (S, G) layout range, at the diag(m) scales and gap pairs on each side of
every encoding step of ScoreLaunch and LaunchTraceback (derived in dp_cases.py's
docstring), in the default form and every forced one, with the counters of
GhostmStageStats saying which kernel the default form chose, and once more
under the two LDS poison patterns. Every comparison is exact.
tests/test_dp_model.py holds the evidence that the model is right and that
these fixtures cannot pass vacuously."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dp_cases as dp
import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import native

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SWEEP = dp.SWEEP_WIDTHS


@pytest.fixture
def stage(data_root):
    """Stage(L) with K1 run where the width seeds; freed after the test."""
    made = []

    def make(L):
        fx = dp.fixture(data_root, L)
        st = dp.Stage(fx)
        if L >= dp.SEED_K:
            st.search(len(fx.candidates()[0]))
        made.append(st)
        return st
    yield make
    for st in made:
        st.close()


# ------------------------------------------------------------ K1
@pytest.mark.parametrize("L", dp.K2_WIDTHS + [100])
def test_candidates_equal_oracle(L, data_root):
    fx = dp.fixture(data_root, L)
    want_qid, want_start = fx.candidates()
    st = dp.Stage(fx)
    qid, start = st.search(len(want_qid))
    st.close()
    assert np.array_equal(qid, want_qid) and np.array_equal(start, want_start)


# ------------------------------------------------------------ K2
@pytest.mark.parametrize("L", dp.K2_WIDTHS)
def test_k2_layouts(L, data_root, stage):
    """Both ends of every layout range: BLOSUM62, PAM250 and diag(11) in every
    form; the all-negative and all-zero matrices (score 0, end = the window's
    last residue column) and zero gap penalties in the default form."""
    st = stage(L)
    for mname in dp.WIDTH_MATRICES:
        dp.check_k2(st, data_root, L, mname)
    for mname in ("neg", "zero"):
        dp.check_k2(st, data_root, L, mname, forms=[{}, {"GHOSTM_K2": "int32"}, {"GHOSTM_K2": "int16"}])
    dp.check_k2(st, data_root, L, "diag11", gaps=(0, 0), forms=[{}])


@pytest.mark.parametrize("m", dp.SCALES)
@pytest.mark.parametrize("L", SWEEP)
def test_k2_scales(L, m, data_root, stage):
    """diag(m) on each side of every step of ScoreLaunch's encoding choice (at
    L = 127; the same scales at an S = 16 and an S = 8 width), every form."""
    d = dp.check_k2(stage(L), data_root, L, f"diag{m}")
    assert d["score_launches"] == 1
    if L == 127:
        assert d["score_launches_packed"] == (1 if m <= 236 else 0)      # L * m < 30000
        assert d["score_launches_swar"] == (1 if m <= 119 else 0)        # 1516 + 2 * 127 m < 0x7C00
        assert d["score_launches_framed"] == (1 if m <= 236 else 0)
        if 120 <= m <= 236:                                              # the f16-number frame, guard 1869
            assert d["score_rechecks"] > 0
        else:
            assert d["score_rechecks"] == 0


@pytest.mark.parametrize("gaps", dp.GAPS, ids=lambda g: f"g{-g[0]}e{-g[1]}")
@pytest.mark.parametrize("L", SWEEP)
def test_k2_gaps(L, gaps, data_root, stage):
    """The gap pairs on each side of the frame limit (sigma_max <= 1000) and of
    the packed limit (-open < 2000), with diag(11)."""
    d = dp.check_k2(stage(L), data_root, L, "diag11", gaps=gaps)
    if L == 127:
        sigma_max = (dp.score_base(L) + 8) * -gaps[1]
        assert d["score_launches_packed"] == (1 if -gaps[0] < 2000 else 0)
        assert d["score_launches_framed"] == (1 if -gaps[0] < 2000 and sigma_max <= 1000 else 0)
    if gaps == (-11, -6) and L == 127:
        assert sigma_max == 1026
    if gaps == (-11, -5) and L == 127:
        assert sigma_max == 855 and d["score_launches_framed"] == 1


# ------------------------------------------------------------ K3
@pytest.mark.parametrize("L", dp.WIDTHS)
def test_k3_layouts(L, data_root, stage):
    """Every candidate's model (qid, end) and the hand-placed ends, windows
    L + 128 and L + 512, every form."""
    st = stage(L)
    for mname in dp.WIDTH_MATRICES:
        for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
            d = dp.check_k3(st, data_root, L, mname, base=base)
            assert d["traceback_launches"] == 1
    dp.check_k3(st, data_root, L, "neg", forms=[{}, {"GHOSTM_K3": "int32"}, {"GHOSTM_K3_SCAN": "0"}])
    dp.check_k3(st, data_root, L, "diag11", gaps=(0, 0), forms=[{}])


@pytest.mark.parametrize("m", dp.SCALES)
@pytest.mark.parametrize("L", SWEEP)
def test_k3_scales(L, m, data_root, stage):
    """diag(m) on each side of the key DP's field limits (hmax < 8000, or 4000
    for the 17-bit key of the wide window) and of the scans' value ranges."""
    st = stage(L)
    hmax = L * m
    for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
        d = dp.check_k3(st, data_root, L, f"diag{m}", base=base)
        if L == 127:
            span = 128 + base
            key = (span < 500 and hmax < 8000) or (span < 1000 and hmax < 4000)
            assert key == (m <= 62 if span == 383 else m <= 31)
            assert d["traceback_launches_key"] == (1 if key else 0)
            assert d["traceback_launches_scan"] == (1 if hmax < 30000 else 0)


@pytest.mark.parametrize("gaps", dp.GAPS, ids=lambda g: f"g{-g[0]}e{-g[1]}")
@pytest.mark.parametrize("L", SWEEP)
def test_k3_gaps(L, gaps, data_root, stage):
    """The gap pairs on each side of the scan's limit (-open < 2000) and of the
    key frame's field test, hmax + (span + 1) * -ext < 8000, with diag(11)."""
    st = stage(L)
    for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
        d = dp.check_k3(st, data_root, L, "diag11", gaps=gaps, base=base)
        if L == 127 and base == 255:
            kframe = L * 11 + (128 + base + 1) * -gaps[1]
            assert d["traceback_launches_key"] == 1
            assert d["traceback_launches_scan"] == (1 if -gaps[0] < 2000 else 0)
            assert d["traceback_launches_keyframe"] == (1 if -gaps[0] < 2000 and kframe < 8000 else 0)
            if gaps[1] in (-17, -18):
                assert kframe == {-17: 7925, -18: 8309}[gaps[1]]


# ------------------------------------------------------------ DB codes 26..31
@pytest.mark.parametrize("L", SWEEP)
def test_db_codes_26_to_31(L, data_root):
    """A chunk whose residues hold the codes 26..31 (SetDbGpu takes any code
    below 32; no formatter writes these), matrix rows 26..31 non-zero: K1 reads
    the index alone; K2 must not run the sparse rows kernel, whose profiles end
    at row 26, nor any packed kernel, which read such a code as END; K3 must
    not scan, as the scan reads it as a zero row. Scores, ends and tracebacks
    equal the model in every form."""
    fx = dp.fixture(data_root, L)
    st = dp.Stage(fx, db=fx.db_codes())
    try:
        qid, start = st.search(len(fx.candidates()[0]))
        assert np.array_equal(qid, fx.candidates()[0]) and np.array_equal(start, fx.candidates()[1])
        d = dp.check_k2(st, data_root, L, "diag11x", codes=True)
        assert d["score_launches"] == 1 and d["score_launches_sparse"] == 0 and d["score_launches_packed"] == 0
        for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
            d = dp.check_k3(st, data_root, L, "diag11x", base=base, codes=True)
            assert d["traceback_launches"] == 1 and d["traceback_launches_scan"] == 0
    finally:
        st.close()


# ------------------------------------------------------------ the detail passes at the same widths
@pytest.mark.parametrize("L", dp.WIDTHS)
def test_ext_and_path_layouts(L, data_root):
    """TraceBackExtGpu and TraceBackPathGpu at both ends of every layout range,
    against their host models, on the oracle's first 60 hits (L = 1, which
    does not seed: the hand-placed hits with the model's starts)."""
    fx = dp.fixture(data_root, L)
    base = dp.trace_base(L)
    if L >= dp.SEED_K:
        tb = np.ascontiguousarray(fx.oracle()[1][:60])
        assert len(tb) >= 30
    else:
        (qid, end), (start, alen, match) = dp.model_traces(data_root, L, "blosum62")
        tb = np.ascontiguousarray(np.stack([qid, end, start, alen, match], axis=1).astype(np.uint32))
    chunk = (fx.nq, fx.L, fx.qseq, fx.db, fx.pos)
    lib = native.load()
    w_start, alen, match, ext = tx.stage_check(lib, fx.d, chunk, tb, tx.blosum62(), base)
    assert np.array_equal(w_start, tb[:, 2]) and np.array_equal(alen, tb[:, 3]) and np.array_equal(match, tb[:, 4])
    tx.check_invariants(alen, match, ext)
    tp.stage_check(lib, fx.d, chunk, tb, tx.blosum62(), base)


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_layout_sweep_under_lds_poison(pattern, data_root):
    """The default-form layout sweep (K1, K2, K3 at every width) in a fresh
    process on the LDS poison build: a result that depended on LDS its kernel
    never wrote would differ from the model under one of the two patterns."""
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    for L in dp.WIDTHS:  # fixtures, dumps and model results are made here, read by the child
        for mname in dp.WIDTH_MATRICES:
            for base in (dp.trace_base(L), dp.trace_base(L, region=64)):
                dp.model_traces(data_root, L, mname, base=base)
    dp.save_models(data_root)
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "dp_poison_child.py"), data_root],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["candidates"] >= 200 * len(dp.K2_WIDTHS) and res["hits"] > res["candidates"]
