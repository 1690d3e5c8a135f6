"""The aligned residue rows on the device: k_path_rows at the stage level
(PathRowsGpu against the host model, hand-made paths included), in batches, the
refused calls, the session post-pass (Session.hits_rows), the -y 8 and -y 9
output, shards, the CLI, a replaced query set and the kernel under the LDS
poison build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import pathrows_cases as pr
import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import native, rows_of
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
ROW_STATS = ("seconds_path_rows", "path_rows_launches", "path_rows_columns", "path_rows_bytes")


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
@pytest.mark.parametrize("L,matrix,gaps", [
    (24, "blosum62", (-11, -1)),
    (75, "blosum62", (-11, -1)),
    (127, "blosum62", (-11, -1)),
    (75, "pam250", (-14, -2)),
], ids=["L24", "L75", "L127", "L75_pam250_g14e2"])
def test_stage_equals_host_model(L, matrix, gaps, data_root):
    """60, 1 and 0 hits of the indel fixture: records and bytes, guard bytes intact."""
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, L, matrix, gaps)
    assert pr.stage_check(native.load(), d, chunk, M, qid, rec, ops, *gaps) == 61


def test_stage_hand_made_paths(data_root):
    """0, 1, 63, 64, 65 and 129 columns, a run longer than a wave, 72, 80 and
    130 one-column runs, the chunk's last residue, position 1, the last record."""
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    qid, rec, ops = pr.hand_paths(nq, L, len(dbseq))
    lib = native.load()
    M = tx.blosum62()
    assert pr.stage_check(lib, d, chunk, M, qid, rec, ops) == len(qid) + 1
    # every hit alone and the hits in reverse order: a wave's result does not depend on its neighbours
    tp.stage_setup(lib, d, chunk, M)
    host, gpu = pr.host_call(lib, chunk, M), pr.gpu_call(lib, L)
    for sel in [[h] for h in range(len(qid))] + [list(range(len(qid)))[::-1]]:
        w_out, w_rows = pr.rows_via(host, qid[sel], rec[sel], ops)
        g_out, g_rows = pr.rows_via(gpu, qid[sel], rec[sel], ops)
        assert np.array_equal(g_out, w_out) and np.array_equal(g_rows, w_rows), sel
    assert lib.FreeGpu() == 0


def test_stage_in_batches(data_root):
    """GHOSTM_ROWS_BATCH_HITS=7 cuts the 60 hits into nine batches and a 1 MB
    budget is honoured too: the same bytes."""
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, 75)
    lib = native.load()
    want = pr.rows_via(pr.host_call(lib, chunk, M), qid, rec, ops)
    tp.stage_setup(lib, d, chunk, M)
    for env in ({"GHOSTM_ROWS_BATCH_HITS": "7"}, {"GHOSTM_ROWS_SCRATCH_MB": "1", "GHOSTM_ROWS_BATCH_HITS": "50"}):
        with _Env(env):
            out, rows = pr.rows_via(pr.gpu_call(lib, 75), qid, rec, ops)
            assert np.array_equal(out, want[0]) and np.array_equal(rows, want[1]), env
    assert lib.FreeGpu() == 0


def test_stage_refusals(data_root):
    """The host model's refusals; the outputs and *rows_used stay untouched."""
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    lib = native.load()
    tp.stage_setup(lib, d, chunk, tx.blosum62())
    pr.check_refusals(pr.gpu_call(lib, L), nq, L, len(dbseq))
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ session
def _run(d, opts, env=None, shard=None, out="x", rows=True):
    with _Env(env):
        with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.path.join(d, out), "-D", "0"] + list(opts),
                     shard=shard) as s:
            s.run()
            res = dict(text=s.output(), hits=s.hits(), stats_before=s.stats())
            if rows:
                res["rec"], res["rows"] = s.hits_rows()
                res["stats"] = s.stats()
                res["again"] = s.hits_rows()
                res["stats_again"] = s.stats()
                res["path"] = s.hits_path()
                res["ext"] = s.hits_ext()
                res["hits_after"] = s.hits()
                res["text_after"] = s.output()
            return res


def _check_session(d, res, M=None):
    M = tx.blosum62() if M is None else M
    hits, rec, rows = res["hits"], res["rec"], res["rows"]
    assert len(hits) == len(rec) > 0
    ext_want, inputs = tx.session_expected(d, hits, M, _base)
    path_want = tp.session_expected(d, hits, inputs, M, _base)
    assert np.array_equal(res["ext"], ext_want)
    assert np.array_equal(res["path"][0], path_want[0]) and np.array_equal(res["path"][1], path_want[1])
    want_rec, want_rows = pr.session_rows_expected(d, hits, inputs, res["path"][0], res["path"][1], M)
    assert np.array_equal(rec, want_rec)
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(rec["rescore"].astype(np.int64), res["path"][0]["score"].astype(np.int64))
    # computed on first use, kept afterwards; the hits and the text untouched
    assert np.array_equal(res["again"][0], rec) and np.array_equal(res["again"][1], rows)
    st = res["stats"]
    assert st["path_rows_launches"] >= 1 and st["seconds_path_rows"] > 0
    assert st["path_rows_columns"] == int(rec["columns"].sum()) and st["path_rows_bytes"] == len(rows)
    for f in ROW_STATS:
        assert res["stats_again"][f] == st[f], f
    assert np.array_equal(res["hits_after"], hits) and res["text_after"] == res["text"]
    return inputs


@pytest.mark.parametrize("ds,opts", [
    ("syn_small", []),
    ("syn_dna", []),                    # name groups of six frames
    ("syn_chunks", ["-b", "1"]),        # 2 query x 3 DB chunks
], ids=["syn_small", "syn_dna", "syn_chunks"])
def test_session_rows_equal_host_model(ds, opts, dataset):
    d = dataset(ds)
    res = _run(d, opts)
    for f in ROW_STATS:  # nothing new runs until the rows are asked for
        assert res["stats_before"][f] == 0, f
    inputs = _check_session(d, res)
    qs, dbs = tx.dataset_chunks(d)
    assert res["rec"]["query_record"].tolist() == [qs[i[0]][0] + i[1] for i in inputs]
    if ds == "syn_chunks":  # every (query chunk, DB chunk) pair has hits: one call each
        assert len({(i[0], i[2]) for i in inputs}) == 6
        assert res["stats"]["path_rows_launches"] == 6
    if ds == "syn_dna":     # every frame occurs, and the record is not always the group's last one
        assert set((res["rec"]["query_record"] % 6).tolist()) == set(range(6))
        assert (res["rec"]["query_record"] != res["hits"]["query_id"]).any()


# ------------------------------------------------------------ -y 8, -y 9
@pytest.fixture(scope="module")
def fixture_runs(data_root):
    d = tx.build_fixture(data_root, 75)
    plain = {y: _run(d, ["-y", y] if y != "0" else [], rows=False)["text"] for y in ("0", "6", "7")}
    return d, plain, {y: _run(d, ["-y", y] if y != "0" else []) for y in ("0", "6", "7", "8", "9")}


def test_y8_lines_column_by_column(fixture_runs):
    d, plain, runs = fixture_runs
    y7, y8 = runs["7"], runs["8"]
    _check_session(d, y8)
    assert y8["stats_before"]["path_rows_launches"] == 1  # -y 8 made the rows in the run
    l7, l8 = y7["text"].split(b"\n"), y8["text"].split(b"\n")
    assert l7[-1] == b"" and l8[-1] == b"" and len(l7) == len(l8) == len(y8["hits"]) + 1 > 40
    rec, rows = y8["rec"], y8["rows"]
    gapped = 0
    for i, (a, b) in enumerate(zip(l7[:-1], l8[:-1])):
        c8 = b.split(b"\t")
        assert len(c8) == 16 and b.startswith(a + b"\t"), i
        q, mid, s = rows_of(rec, rows, i)
        assert c8[13:] == [str(int(rec["positives"][i])).encode(), q, s], i
        gapped += b"-" in q or b"-" in s
    assert gapped >= 20
    for y in ("0", "6", "7", "9"):  # the same hits and rows for any -y
        assert np.array_equal(runs[y]["hits"], y8["hits"])
        assert np.array_equal(runs[y]["rec"], rec) and np.array_equal(runs[y]["rows"], rows)


def test_y9_blocks(fixture_runs):
    d, plain, runs = fixture_runs
    y8, y9 = runs["8"], runs["9"]
    rec, rows = y9["rec"], y9["rows"]
    path = y9["path"][0]
    lines = y9["text"].split(b"\n")
    assert len(lines) == 5 * len(rec) + 1 and lines[-1] == b""
    for i, l8 in enumerate(y8["text"].split(b"\n")[:-1]):
        q, mid, s = rows_of(rec, rows, i)
        num = lambda v: str(int(v)).encode()  # noqa: E731
        assert lines[5 * i:5 * i + 5] == [
            b"# " + b"\t".join(l8.split(b"\t")[:14]),
            b"\t".join([b"Query", num(path["q_start"][i] + 1), q, num(path["q_end"][i] + 1)]),
            b"\t\t" + mid + b"\t",
            b"\t".join([b"Sbjct", num(path["s_start"][i] + 1), s, num(path["s_end"][i] + 1)]),
            b"",
        ], i


def test_y0_y6_y7_keep_their_bytes(fixture_runs, tmp_path):
    """The text of -y 0, 6 and 7 does not depend on the rows being asked for,
    and -y 0 is still the oracle's."""
    d, plain, runs = fixture_runs
    for y in ("0", "6", "7"):
        assert runs[y]["text"] == plain[y] == runs[y]["text_after"], y
        assert runs[y]["stats_before"]["path_rows_launches"] == 0
    assert cases.run_aln(cases.ORACLE, d, [], {}, str(tmp_path / "o.out")) == plain["0"]
    for a, b in zip(plain["6"].split(b"\n")[:-1], plain["7"].split(b"\n")[:-1]):
        assert len(a.split(b"\t")) == 12 and len(b.split(b"\t")) == 13


def test_session_in_batches(fixture_runs):
    """GHOSTM_ROWS_BATCH_HITS=7: the same records, bytes and text, and
    path_rows_launches shows that the batches ran."""
    d, plain, runs = fixture_runs
    y8 = runs["8"]
    n = len(y8["hits"])
    for env, launches in (({"GHOSTM_ROWS_BATCH_HITS": "7"}, (n + 6) // 7),
                          ({"GHOSTM_ROWS_SCRATCH_MB": "1", "GHOSTM_ROWS_BATCH_HITS": "50"}, (n + 49) // 50)):
        res = _run(d, ["-y", "8"], env=env)
        assert y8["stats"]["path_rows_launches"] == 1 and res["stats"]["path_rows_launches"] == launches
        assert launches > 5 or "GHOSTM_ROWS_SCRATCH_MB" in env
        assert res["text"] == y8["text"]
        assert np.array_equal(res["rec"], y8["rec"]) and np.array_equal(res["rows"], y8["rows"])
        assert res["stats"]["path_rows_bytes"] == y8["stats"]["path_rows_bytes"]


def test_shards_concatenate_to_the_unsharded_result(fixture_runs):
    d, plain, runs = fixture_runs
    y8 = runs["8"]
    parts = [_run(d, ["-y", "8"], shard=(r, 3)) for r in range(3)]
    assert all(len(p["hits"]) > 0 for p in parts)
    assert b"".join(p["text"] for p in parts) == y8["text"]
    recs, at = [], 0
    for p in parts:
        r = p["rec"].copy()
        r["rows_offset"] += at
        at += len(p["rows"])
        recs.append(r)
    assert np.array_equal(np.concatenate(recs), y8["rec"])
    assert np.array_equal(np.concatenate([p["rows"] for p in parts]), y8["rows"])


def test_cli_writes_the_session_bytes(fixture_runs, tmp_path):
    d, plain, runs = fixture_runs
    for y in ("8", "9"):
        assert cases.run_aln(cases.GHOSTM, d, ["-y", y, "-D", "0"], {}, str(tmp_path / f"cli{y}.out")) == runs[y]["text"]
    out2 = tmp_path / "session.out"
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", str(out2), "-D", "0", "-y", "8"]) as s:
        s.run(to_file=True)
        s.write()  # a no-op after the run wrote the file
    assert out2.read_bytes() == runs["8"]["text"]


def test_cli_unsupported_score_option(tmp_path):
    """-y 8 and -y 9 price hits like -y 0: an unknown matrix/gap combination is
    the reference's error, printed, exit status 0."""
    for y in ("8", "9"):
        r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", str(tmp_path / "o"), "-y", y, "-G", "5"],
                           capture_output=True)
        assert r.returncode == 0
        assert b"not support score option" in r.stderr
        assert not (tmp_path / "o").exists()


# ------------------------------------------------------------ a replaced query set
def test_rows_follow_a_replaced_query_set(data_root):
    """The fixture's reads of 75, then its reads of 24 (the same subjects) set
    from FASTA on the live session: hits_rows() is the new set's."""
    d75, d24 = tx.build_fixture(data_root, 75), tx.build_fixture(data_root, 24)
    assert open(f"{d75}/db.fa").read() == open(f"{d24}/db.fa").read()
    want = {d: _run(d, []) for d in (d75, d24)}
    with Session.for_db(["-d", f"{d75}/db", "-o", os.devnull, "-D", "0"]) as s:
        for d, width in ((d75, 75), (d24, 24), (d75, 75)):
            s.set_queries_fasta(f"{d}/q.fa", width=width)
            for f in ROW_STATS:
                assert s.stats()[f] == 0, f
            s.run()
            assert s.hits().tobytes() == want[d]["hits"].tobytes()
            rec, rows = s.hits_rows()
            assert np.array_equal(rec, want[d]["rec"]) and np.array_equal(rows, want[d]["rows"])
    assert not np.array_equal(want[d75]["rows"], want[d24]["rows"])


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern, data_root):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    pr.fixture_paths(data_root, 75)  # built here, read by the child
    pr.build_tiny(data_root)
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "pathrows_poison_child.py"), data_root],
                       capture_output=True, text=True, timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["hits"] == 61 + 14
