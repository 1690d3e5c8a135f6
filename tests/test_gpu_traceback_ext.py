"""The extended traceback on the device: k_traceback_ext at the stage level
(TraceBackExtGpu against the host model and K3), the session post-pass
(Session.hits_ext), the BLAST-tabular output (-y 6), shards, the CLI, and the
kernel under the LDS poison build."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import tbext_cases as tx
from ghostm_amd import native
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")


def _base(L, region=16, extend=2):
    return L + 2 * extend * 2 * region


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("L,opts,region,matrix,gaps", [
    (24, (), 16, "blosum62", (-11, -1)),    # S = 8, three lanes per hit
    (40, (), 16, "blosum62", (-11, -1)),    # S = 8, five lanes
    (75, (), 16, "blosum62", (-11, -1)),    # S = 16, five lanes
    (127, (), 16, "blosum62", (-11, -1)),   # S = 16, eight lanes
    (75, ("-r", "64"), 64, "blosum62", (-11, -1)),
    (75, ("-M", cases.PAM250, "-G", "14", "-E", "2"), 16, "pam250", (-14, -2)),
], ids=["L24", "L40", "L75", "L127", "L75_r64", "L75_pam250_g14e2"])
def test_stage_equals_host_model(L, opts, region, matrix, gaps, data_root):
    d, chunk, tb = tx.fixture_hits(data_root, L, opts)
    M = tx.blosum62() if matrix == "blosum62" else tx.pam250()
    start, alen, match, ext = tx.stage_check(native.load(), d, chunk, tb, M, _base(L, region), gaps[0], gaps[1])
    if not opts:
        tx.assert_gapped(alen, match, ext)
    tx.check_invariants(alen, match, ext)


def test_stage_refuses_what_the_fields_cannot_hold(data_root):
    """A window wider than the packed gap-open field is an error, not a wrapped value."""
    d, chunk, tb = tx.fixture_hits(data_root, 24)
    lib = native.load()
    tx.stage_check(lib, d, chunk, tb[:1], tx.blosum62(), _base(24))
    nq, L, qseq, dbseq, pos = chunk
    M = tx.blosum62()
    assert lib.SetOptionGpu(1 << 27, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0) == 0
    assert lib.SetQueryGpu(tx._p(qseq, ctypes.c_uint8), nq, L) == 0
    seed, kc, ipos = tx.load_index(d)
    assert lib.SetDbGpu(tx._p(dbseq, ctypes.c_uint8), len(dbseq), tx._p(kc), len(kc), tx._p(ipos), len(ipos)) == 0
    qid, end = np.ascontiguousarray(tb[:1, 0]), np.ascontiguousarray(tb[:1, 1])
    out = np.zeros(4, dtype=np.uint32)
    rc = lib.TraceBackExtGpu(1, tx._p(qid), tx._p(end), None, L, 40000, -11, -1, tx._p(out), tx._p(out), tx._p(out),
                             None)
    assert rc != 0 and "window" in native.last_error()
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ session
def _run(d, opts, env=None, shard=None, out="x"):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.path.join(d, out), "-D", "0"] + list(opts),
                     shard=shard) as s:
            s.run()
            st0 = s.stats()
            return dict(text=s.output(), hits=s.hits(), stats_before=st0, ext=s.hits_ext(), stats=s.stats())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def small_runs(dataset):
    d = dataset("syn_small")
    return d, _run(d, []), _run(d, ["-y", "6"])


def test_tabular_lines_column_by_column(small_runs):
    d, y0, y6 = small_runs
    l0 = y0["text"].split(b"\n")
    l6 = y6["text"].split(b"\n")
    assert l0[-1] == b"" and l6[-1] == b"" and len(l0) == len(l6) == len(y0["hits"]) + 1 > 100
    ext = y6["ext"]
    for i, (a, b) in enumerate(zip(l0[:-1], l6[:-1])):
        c0 = a.split(b"\t")
        assert len(c0) == 10 and c0[9] == b""  # style 0 ends its lines with a tab
        want = c0[0:4] + [str(int(v)).encode() for v in (ext["mismatches"][i], ext["gap_opens"][i],
                                                        ext["q_start"][i] + 1, ext["q_end"][i] + 1)] + c0[5:9]
        assert b.split(b"\t") == want, i
    assert np.array_equal(y0["hits"], y6["hits"])
    assert np.array_equal(y0["ext"], y6["ext"])
    # the default path launches nothing new until the records are asked for
    assert y0["stats_before"]["traceback_ext_launches"] == 0 and y0["stats_before"]["traceback_ext_cells"] == 0
    assert y0["stats"]["traceback_ext_launches"] >= 1 and y0["stats"]["traceback_ext_cells"] > 0
    assert y6["stats_before"]["traceback_ext_launches"] >= 1
    assert y6["stats"]["traceback_ext_launches"] == y6["stats_before"]["traceback_ext_launches"]  # cached
    alen, match = y6["hits"]["aln_len"], y6["hits"]["aln_match"]
    tx.check_invariants(alen, match, ext)


def _check_session(d, res, M, base_of, gaps=(-11, -1)):
    hits, ext = res["hits"], res["ext"]
    assert len(hits) == len(ext) > 0
    want, inputs = tx.session_expected(d, hits, M, base_of, gaps[0], gaps[1])
    assert np.array_equal(ext, want)
    tx.check_invariants(hits["aln_len"], hits["aln_match"], ext)
    # the Python model on a fixed sample of 100 hits (the DP stopped at the known start)
    qs, dbs = tx.dataset_chunks(d)
    for h in np.unique(np.linspace(0, len(hits) - 1, 100).astype(int)):
        qi, q, di, end, start = inputs[h]
        L = qs[qi][2]
        r = tx.py_model(qs[qi][3][q * L:(q + 1) * L], dbs[di][2], M, end, base_of(L), gaps[0], gaps[1],
                        max_cols=end - start + 1)
        assert (r["start"], r["len"], r["match"]) == (start, hits["aln_len"][h], hits["aln_match"][h])
        assert (r["q_start"], r["q_end"], r["mism"], r["gapopen"]) == tuple(int(x) for x in ext[h]), h
    return inputs


@pytest.mark.parametrize("ds,opts,env", [
    ("syn_dna", [], {}),                                               # name groups of six frames
    ("syn_chunks", ["-b", "1"], {}),                                   # 2 query x 3 DB chunks (7000 of 70000 hits)
    ("syn_small", ["-b", "20"], {"GHOSTM_MAX_LIST_OVERRIDE": "300"}),  # batch cuts, carried lists
    ("syn_small", [], {"GHOSTM_MERGE": "host"}),
], ids=["syn_dna", "syn_chunks", "syn_small_cut300_b20", "syn_small_hostmerge"])
def test_session_records_equal_host_model(ds, opts, env, dataset):
    d = dataset(ds)
    res = _run(d, opts, env)
    inputs = _check_session(d, res, tx.blosum62(), _base)
    if ds == "syn_chunks":  # every (query chunk, DB chunk) pair has hits
        assert len({(i[0], i[2]) for i in inputs}) == 6
    if ds == "syn_dna":     # hits of every frame position of a group, not only the record's query
        assert len({i[1] % 6 for i in inputs}) == 6


def test_session_records_on_the_indel_fixture(data_root):
    d = tx.build_fixture(data_root, 75)
    res = _run(d, ["-y", "6"])
    tx.assert_gapped(res["hits"]["aln_len"], res["hits"]["aln_match"], res["ext"])
    _check_session(d, res, tx.blosum62(), _base)


def test_shards_concatenate_to_the_unsharded_text(small_runs):
    d, y0, y6 = small_runs
    parts = [_run(d, ["-y", "6"], shard=(r, 3)) for r in range(3)]
    assert all(len(p["hits"]) > 0 for p in parts)
    assert b"".join(p["text"] for p in parts) == y6["text"]
    assert np.array_equal(np.concatenate([p["ext"] for p in parts]), y6["ext"])


def test_cli_and_run_to_file_write_the_same_bytes(small_runs, tmp_path):
    d, y0, y6 = small_runs
    out = tmp_path / "cli.out"
    assert cases.run_aln(cases.GHOSTM, d, ["-y", "6", "-D", "0"], {}, str(out)) == y6["text"]
    out2 = tmp_path / "session.out"
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", str(out2), "-D", "0", "-y", "6"]) as s:
        s.run(to_file=True)
        s.write()  # a no-op after the run wrote the file
        assert s.output() == y6["text"]
    assert out2.read_bytes() == y6["text"]


def test_cli_unsupported_score_option(tmp_path):
    """-y 6 prices hits like -y 0: an unknown matrix/gap combination is the
    reference's error (statistics.cpp:143-145), printed, exit status 0."""
    r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", str(tmp_path / "o"), "-y", "6", "-G", "5"],
                       capture_output=True)
    assert r.returncode == 0
    assert b"not support score option" in r.stderr
    assert not (tmp_path / "o").exists()


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern, data_root):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    tx.fixture_hits(data_root, 75)  # built here, read by the child
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "tbext_poison_child.py"), data_root],
                       capture_output=True, text=True, timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
