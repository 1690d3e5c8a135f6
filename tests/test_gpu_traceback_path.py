"""The alignment paths on the device: k_tb_path_fill, k_tb_path_walk and
k_ops_compact at the stage level (TraceBackPathGpu against the host model), in
batches, the session post-pass (Session.hits_path), the -y 7 output, shards,
the CLI, and the kernels under the LDS poison build."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import cigar, native, traceback_path_host
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")


def _base(L, region=16, extend=2):
    return L + 2 * extend * 2 * region


class _Env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("L,opts,region,matrix,gaps", [
    (24, (), 16, "blosum62", (-11, -1)),    # three lanes per hit
    (40, (), 16, "blosum62", (-11, -1)),
    (75, (), 16, "blosum62", (-11, -1)),
    (127, (), 16, "blosum62", (-11, -1)),   # the widest group
    (75, ("-r", "64"), 64, "blosum62", (-11, -1)),
    (75, ("-M", cases.PAM250, "-G", "14", "-E", "2"), 16, "pam250", (-14, -2)),
    (127, tp.RUNS, 16, "blosum62", (-11, -1)),  # slots of more than 64 words and of none in one batch
], ids=["L24", "L40", "L75", "L127", "L75_r64", "L75_pam250_g14e2", "L127_runs"])
def test_stage_equals_host_model(L, opts, region, matrix, gaps, data_root):
    """With and without the known starts, on all hits, 1 and 0 hits; reads 0 to
    3 of the fixture cover the window clipped at DB position 0 and the END
    break, tp.runs_hits the compaction (k_ops_compact: one wave per slot, 64
    words at a time)."""
    d, chunk, tb = (tp.runs_hits(data_root, L, _base(L, region)) if opts is tp.RUNS
                    else tx.fixture_hits(data_root, L, opts))
    M = tx.blosum62() if matrix == "blosum62" else tx.pam250()
    rec, ops = tp.stage_check(native.load(), d, chunk, tb, M, _base(L, region), gaps[0], gaps[1])
    if not opts:
        tp.assert_gapped(rec, ops)
    nq, L_, qseq, dbseq, pos = chunk
    for h in range(len(tb)):
        if rec["score"][h] == 0:  # no path to re-walk: only the runs case has such hits
            assert opts is tp.RUNS and rec["n_runs"][h] == 0
            continue
        q = int(tb[h, 0])
        tp.check_path(qseq[q * L:(q + 1) * L], dbseq, M, rec[h], tp.hit_words(rec, ops, h), gaps[0], gaps[1],
                      db_start=tb[h, 2])


def test_stage_in_batches(data_root):
    """GHOSTM_PATH_BATCH_HITS=7 cuts the 60 hits into nine batches and a 1 MB
    budget is honoured too: the same bytes."""
    L = 75
    d, chunk, tb = tx.fixture_hits(data_root, L)
    nq, L_, qseq, dbseq, pos = chunk
    lib = native.load()
    M = tx.blosum62()
    qid, end, starts = (np.ascontiguousarray(tb[:, c]) for c in range(3))
    want = traceback_path_host(qseq, L, dbseq, M, qid, end, _base(L))
    tp.stage_setup(lib, d, chunk, M)
    for env in ({"GHOSTM_PATH_BATCH_HITS": "7"}, {"GHOSTM_PATH_SCRATCH_MB": "1", "GHOSTM_PATH_BATCH_HITS": "50"}):
        with _Env(env):
            for s_in in (None, starts):
                rec, ops = tp.gpu_paths(lib, qid, end, s_in, L, _base(L), -11, -1)
                assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert lib.FreeGpu() == 0


def test_stage_refusals(data_root):
    d, chunk, tb = tx.fixture_hits(data_root, 24)
    nq, L, qseq, dbseq, pos = chunk
    lib = native.load()
    tp.stage_setup(lib, d, chunk, tx.blosum62())
    qid, end = np.ascontiguousarray(tb[:1, 0]), np.ascontiguousarray(tb[:1, 1])
    used = ctypes.c_size_t(0)
    rc = lib.TraceBackPathGpu(1, tx._p(qid), tx._p(end), None, L, 40000, -11, -1, None, None, 0, ctypes.byref(used))
    assert rc != 0 and "window" in native.last_error()
    rc = lib.TraceBackPathGpu(1, tx._p(qid), tx._p(end), None, L + 1, _base(L), -11, -1, None, None, 0,
                              ctypes.byref(used))
    assert rc != 0 and "shape" in native.last_error()
    ops = np.full(4, 0xDEADBEEF, dtype=np.uint32)
    qid, end = np.ascontiguousarray(tb[:, 0]), np.ascontiguousarray(tb[:, 1])
    rc = lib.TraceBackPathGpu(len(qid), tx._p(qid), tx._p(end), None, L, _base(L), -11, -1, None, tx._p(ops), 2,
                              ctypes.byref(used))
    assert rc != 0 and "ops_cap" in native.last_error() and (ops == 0xDEADBEEF).all()
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ session
def _run(d, opts, env=None, shard=None, out="x", to_file=False):
    with _Env(env):
        with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.path.join(d, out), "-D", "0"] + list(opts),
                     shard=shard) as s:
            s.run(to_file=to_file)
            st0 = s.stats()
            text, hits = s.output(), s.hits()
            rec, ops = s.hits_path()
            st1 = s.stats()
            rec2, ops2 = s.hits_path()
            return dict(text=text, hits=hits, stats_before=st0, rec=rec, ops=ops, stats=st1, stats_again=s.stats(),
                        again=(rec2, ops2), ext=s.hits_ext(), hits_after=s.hits())


PATH_STATS = ("seconds_traceback_path", "traceback_path_launches", "traceback_path_cells", "traceback_path_dir_bytes")


def _check_session(d, res, M, base_of, gaps=(-11, -1)):
    hits, rec, ops = res["hits"], res["rec"], res["ops"]
    assert len(hits) == len(rec) > 0
    ext_want, inputs = tx.session_expected(d, hits, M, base_of, gaps[0], gaps[1])
    assert np.array_equal(res["ext"], ext_want)
    want_rec, want_ops = tp.session_expected(d, hits, inputs, M, base_of, gaps[0], gaps[1])
    assert np.array_equal(rec, want_rec)
    assert np.array_equal(ops, want_ops)
    tp.check_session_invariants(d, hits, res["ext"], rec, ops, inputs, M, gaps[0], gaps[1])
    assert np.array_equal(rec["s_start"], hits["db_start"])
    # computed on first use, kept afterwards, the hits untouched
    assert np.array_equal(res["again"][0], rec) and np.array_equal(res["again"][1], ops)
    assert res["stats"]["traceback_path_launches"] >= 1 and res["stats"]["traceback_path_cells"] > 0
    assert res["stats"]["traceback_path_dir_bytes"] > 0
    for f in PATH_STATS:
        assert res["stats_again"][f] == res["stats"][f], f
    assert np.array_equal(res["hits_after"], hits)
    return inputs


@pytest.mark.parametrize("ds,opts", [
    ("syn_small", []),
    ("syn_dna", []),                    # name groups of six frames
    ("syn_chunks", ["-b", "1"]),        # 2 query x 3 DB chunks
], ids=["syn_small", "syn_dna", "syn_chunks"])
def test_session_paths_equal_host_model(ds, opts, dataset):
    d = dataset(ds)
    res = _run(d, opts)
    for f in PATH_STATS:  # the default path launches nothing new until the paths are asked for
        assert res["stats_before"][f] == 0, f
    inputs = _check_session(d, res, tx.blosum62(), _base)
    if ds == "syn_chunks":  # every (query chunk, DB chunk) pair has hits: one call each
        assert len({(i[0], i[2]) for i in inputs}) == 6
        assert res["stats"]["traceback_path_launches"] == 6
    if ds == "syn_dna":     # hits of every frame position of a group, not only the record's query
        assert len({i[1] % 6 for i in inputs}) == 6


def test_session_paths_on_the_indel_fixture(data_root):
    d = tx.build_fixture(data_root, 75)
    res = _run(d, ["-y", "7"])
    tp.assert_gapped(res["rec"], res["ops"])
    assert res["stats_before"]["traceback_path_launches"] >= 1  # -y 7 made them in the run
    _check_session(d, res, tx.blosum62(), _base)


# ------------------------------------------------------------ -y 7
@pytest.fixture(scope="module")
def fixture_runs(data_root):
    d = tx.build_fixture(data_root, 75)
    return d, _run(d, []), _run(d, ["-y", "6"]), _run(d, ["-y", "7"])


def _id_text(matches, length):
    """pident as style 0 prints it: float 100 * (matches / length), %g."""
    v = np.float32(np.float32(matches) / np.float32(length)) * np.float32(100)
    return ("%g" % float(np.float32(v))).encode()


def test_y7_lines_column_by_column(fixture_runs):
    d, y0, y6, y7 = fixture_runs
    l6 = y6["text"].split(b"\n")
    l7 = y7["text"].split(b"\n")
    assert l6[-1] == b"" and l7[-1] == b"" and len(l6) == len(l7) == len(y7["hits"]) + 1 > 40
    rec, ops = y7["rec"], y7["ops"]
    gapped = 0
    for i, (a, b) in enumerate(zip(l6[:-1], l7[:-1])):
        c6, c7 = a.split(b"\t"), b.split(b"\t")
        assert len(c6) == 12 and len(c7) == 13
        assert c7[0:2] == c6[0:2] and c7[10:12] == c6[10:12]
        s = tp.expand(tp.hit_words(rec, ops, i))
        n = {c: s.count(c) for c in tp.OPS}
        gap_runs = sum(1 for w in tp.hit_words(rec, ops, i) if int(w) & 2)
        gapped += gap_runs > 0
        want = [_id_text(n["="], len(s))] + [str(int(v)).encode() for v in (
            len(s), n["X"], gap_runs, rec["q_start"][i] + 1, rec["q_end"][i] + 1, rec["s_start"][i] + 1,
            rec["s_end"][i] + 1)]
        assert c7[2:10] == want, (i, c7, want)
        assert c7[12] == cigar(tp.hit_words(rec, ops, i)).encode()
    assert gapped >= 20
    # -y 6 and -y 0 of the same session setup are what they were, the paths the same for any -y
    assert np.array_equal(y0["hits"], y7["hits"]) and np.array_equal(y6["hits"], y7["hits"])
    for other in (y0, y6):
        assert np.array_equal(other["rec"], rec) and np.array_equal(other["ops"], ops)
    assert y6["stats_before"]["traceback_path_launches"] == 0 and y0["stats_before"]["traceback_path_launches"] == 0


def test_session_in_batches(fixture_runs):
    """GHOSTM_PATH_BATCH_HITS=7: the same records, words and text, and
    traceback_path_launches shows that the batches ran."""
    d, y0, y6, y7 = fixture_runs
    res = _run(d, ["-y", "7"], env={"GHOSTM_PATH_BATCH_HITS": "7"})
    n = len(y7["hits"])
    assert y7["stats"]["traceback_path_launches"] == 1
    assert res["stats"]["traceback_path_launches"] == (n + 6) // 7 > 5
    assert res["text"] == y7["text"]
    assert np.array_equal(res["rec"], y7["rec"]) and np.array_equal(res["ops"], y7["ops"])
    assert res["stats"]["traceback_path_cells"] == y7["stats"]["traceback_path_cells"]
    assert res["stats"]["traceback_path_dir_bytes"] == y7["stats"]["traceback_path_dir_bytes"]


def test_y6_and_y0_keep_their_bytes(fixture_runs, tmp_path):
    """Against the oracle for -y 0 and, column by column, -y 6 from -y 0 and hits_ext."""
    d, y0, y6, y7 = fixture_runs
    assert cases.run_aln(cases.ORACLE, d, [], {}, str(tmp_path / "o.out")) == y0["text"]
    ext = y6["ext"]
    for i, (a, b) in enumerate(zip(y0["text"].split(b"\n")[:-1], y6["text"].split(b"\n")[:-1])):
        c0 = a.split(b"\t")
        want = c0[0:4] + [str(int(v)).encode() for v in (ext["mismatches"][i], ext["gap_opens"][i],
                                                        ext["q_start"][i] + 1, ext["q_end"][i] + 1)] + c0[5:9]
        assert b.split(b"\t") == want, i


def test_cli_run_to_file_and_output_write_the_same_bytes(fixture_runs, tmp_path):
    d, y0, y6, y7 = fixture_runs
    out = tmp_path / "cli.out"
    assert cases.run_aln(cases.GHOSTM, d, ["-y", "7", "-D", "0"], {}, str(out)) == y7["text"]
    out2 = tmp_path / "session.out"
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", str(out2), "-D", "0", "-y", "7"]) as s:
        s.run(to_file=True)
        s.write()  # a no-op after the run wrote the file
        assert s.output() == y7["text"]
    assert out2.read_bytes() == y7["text"]


def test_shards_concatenate_to_the_unsharded_text(fixture_runs):
    d, y0, y6, y7 = fixture_runs
    parts = [_run(d, ["-y", "7"], shard=(r, 3)) for r in range(3)]
    assert all(len(p["hits"]) > 0 for p in parts)
    assert b"".join(p["text"] for p in parts) == y7["text"]
    recs, at = [], 0
    for p in parts:
        r = p["rec"].copy()
        r["ops_offset"] += at
        at += len(p["ops"])
        recs.append(r)
    assert np.array_equal(np.concatenate(recs), y7["rec"])
    assert np.array_equal(np.concatenate([p["ops"] for p in parts]), y7["ops"])


def test_cli_unsupported_score_option(tmp_path):
    """-y 7 prices hits like -y 0 and -y 6: an unknown matrix/gap combination is
    the reference's error, printed, exit status 0."""
    r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", str(tmp_path / "o"), "-y", "7", "-G", "5"],
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
    p = subprocess.run([sys.executable, os.path.join(HERE, "tbpath_poison_child.py"), data_root],
                       capture_output=True, text=True, timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
