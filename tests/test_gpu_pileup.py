"""The subject pile-up on the device: k_pileup and k_pileup_finish at the stage
level (PathPileupGpu against the numpy model and the host model, the tile-edge
shapes with tiles of 32 positions and parts of 7 hits), the refused calls, the
session post-pass (Session.pileup, Session.subject_profile), profile windows of
1 MB, the -y 10 and -y 11 output, shards, the CLI, a replaced query set and the
kernels under the LDS poison build. Every comparison is equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import pathrows_cases as pr
import pileup_cases as pc
import tbext_cases as tx
import tbpath_cases as tp
from ghostm_amd import consensus_text, native
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
PILEUP_STATS = ("seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns")


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("L", [24, 75, 127])
def test_stage_equals_models(L, data_root):
    """60, 1 and 0 hits of the indel fixture, with the profile and with NULL."""
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, L)
    assert pc.stage_check(native.load(), d, chunk, M, qid, rec, ops) == 61


def test_stage_hand_made_paths_and_tile_edges(data_root):
    """The hand-made paths at the default tile, then, with GHOSTM_PILEUP_TILE=32
    and GHOSTM_PILEUP_PART_HITS=7: a path over three tiles, a D run across a
    tile edge, an I run at one, position 1, the chunk's last residue, 300 copies
    of one hit (43 parts of one tile, counts past 255) and the hits reversed."""
    d, chunk = pr.build_tiny(data_root)
    qid, rec, ops = pr.hand_paths(chunk[0], chunk[1], len(chunk[3]))
    assert pc.stage_check(native.load(), d, chunk, tx.blosum62(), qid, rec, ops, counts=(len(qid),), edges=True) == \
        len(qid) + 325


def test_stage_small_tiles_and_windows_on_the_fixture(data_root):
    """The fixture's 60 hits with tiles of 32 and 100 positions, parts of 1 and 7
    hits, upload batches of 7 hits and one tile per window: the same arrays."""
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, 75)
    nq, L, qseq, dbseq, pos = chunk
    lib = native.load()
    want = pc.model(qseq, L, dbseq, qid, rec, ops)
    tp.stage_setup(lib, d, chunk, M)
    gpu = pc.gpu_call(lib, L)
    for env in ({"GHOSTM_PILEUP_TILE": "32", "GHOSTM_PILEUP_PART_HITS": "1"},
                {"GHOSTM_PILEUP_TILE": "100", "GHOSTM_PILEUP_PART_HITS": "7", "GHOSTM_PILEUP_BATCH_HITS": "7"},
                {"GHOSTM_PILEUP_TILE": "1", "GHOSTM_PILEUP_PART_HITS": "3"},      # clamped to 32
                {"GHOSTM_PILEUP_TILE": "4096"}):                                 # clamped to the compiled maximum
        with pc.pr_env(env):
            pc.assert_same(pc.pileup_via(gpu, qid, rec, ops, len(dbseq)), want, env)
    assert lib.FreeGpu() == 0


def test_stage_refusals(data_root):
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    lib = native.load()
    tp.stage_setup(lib, d, chunk, tx.blosum62())
    pc.check_refusals(pc.gpu_call(lib, L), nq, L, len(dbseq), gpu=True)
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ session
def _run(d, opts, env=None, shard=None, out="x", pile=True, profiles=0):
    with pc.pr_env(env):
        with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.path.join(d, out), "-D", "0"] + list(opts),
                     shard=shard) as s:
            s.run()
            res = dict(text=s.output(), hits=s.hits(), stats_before=s.stats())
            if pile:
                res["pile"] = s.pileup()
                res["stats"] = s.stats()
                res["again"] = s.pileup()
                res["stats_again"] = s.stats()
                res["path"] = s.hits_path()
                res["rows"] = s.hits_rows()[0]
                res["hits_after"] = s.hits()
                res["text_after"] = s.output()
                ids = np.unique(res["hits"]["db_id"])[:profiles]
                res["profiles"] = {int(i): s.subject_profile(int(i)) for i in ids}
            return res


def _check_session(d, res):
    hits = res["hits"]
    subj, depth, ident, cons = res["pile"]
    assert len(hits) > 0
    want = pc.session_model(d, hits, res["rows"]["query_record"], res["path"][0], res["path"][1])
    assert np.array_equal(subj, want[0])
    pc.assert_same((depth, ident, cons), want[1:4], "session")
    assert np.array_equal(subj["hits"], np.bincount(hits["db_id"], minlength=len(subj)))
    assert int(subj["identities_sum"].sum()) == int(res["rows"]["identities"].sum())
    st = res["stats"]
    assert st["pileup_launches"] >= 1 and st["pileup_windows"] >= 1 and st["pileup_parts"] >= st["pileup_launches"]
    assert st["seconds_pileup"] > 0 and st["pileup_columns"] == int(subj["depth_sum"].sum()) == int(depth.sum())
    for a, b in zip(res["again"], res["pile"]):
        assert np.array_equal(a, b)
    for f in PILEUP_STATS:  # computed on first use, kept afterwards
        assert res["stats_again"][f] == st[f], f
    assert np.array_equal(res["hits_after"], hits) and res["text_after"] == res["text"]
    for i, prof in res["profiles"].items():
        a, n = int(subj["offset"][i]), int(subj["length"][i])
        assert prof.shape == (n, 32) and np.array_equal(prof, want[4][a:a + n])
        assert np.array_equal(prof.sum(axis=1), depth[a:a + n])
    return want


@pytest.mark.parametrize("ds,opts", [
    ("syn_small", []),
    ("syn_dna", []),                    # name groups of six frames
    ("syn_chunks", ["-b", "1"]),        # 2 query x 3 DB chunks
], ids=["syn_small", "syn_dna", "syn_chunks"])
def test_session_pileup_equals_numpy_model(ds, opts, dataset):
    d = dataset(ds)
    res = _run(d, opts, profiles=4)
    for f in PILEUP_STATS:  # nothing new runs until the pile-up is asked for
        assert res["stats_before"][f] == 0, f
    _check_session(d, res)
    if ds == "syn_chunks":  # per DB chunk one window, in it one launch per query chunk
        assert res["stats"]["pileup_windows"] == 3 and res["stats"]["pileup_launches"] == 6


def test_session_windows_of_one_megabyte(dataset):
    """GHOSTM_PILEUP_SCRATCH_MB=1 holds 8192 positions: syn_small's chunk of
    200 000 residues takes 25 windows and gives the same arrays; small tiles and
    parts too."""
    d = dataset("syn_small")
    base = _run(d, [])
    assert base["stats"]["pileup_windows"] == 1
    for env in ({"GHOSTM_PILEUP_SCRATCH_MB": "1"},
                {"GHOSTM_PILEUP_SCRATCH_MB": "1", "GHOSTM_PILEUP_TILE": "96", "GHOSTM_PILEUP_PART_HITS": "2",
                 "GHOSTM_PILEUP_BATCH_HITS": "100"}):
        res = _run(d, [], env=env)
        assert res["stats"]["pileup_windows"] >= 3
        for a, b in zip(res["pile"], base["pile"]):
            assert np.array_equal(a, b), env
        assert res["stats"]["pileup_columns"] == base["stats"]["pileup_columns"]
    assert res["stats"]["pileup_parts"] > base["stats"]["pileup_parts"]


# ------------------------------------------------------------ -y 10, -y 11, shards, the CLI
@pytest.fixture(scope="module")
def fixture_runs(data_root):
    d = tx.build_fixture(data_root, 75)
    plain = {y: _run(d, ["-y", y] if y != "0" else [], pile=False)["text"] for y in ("0", "7")}
    return d, plain, {y: _run(d, ["-y", y] if y != "0" else []) for y in ("0", "7", "10", "11")}


def test_y10_y11_lines_column_by_column(fixture_runs):
    d, plain, runs = fixture_runs
    _check_session(d, runs["10"])
    names = [x for c in range(len(tx.dataset_chunks(d)[1])) for x in open(f"{d}/db_{c}.nam").read().split("\n") if x]
    for y in ("10", "11"):
        subj, depth, ident, cons = runs[y]["pile"]
        assert runs[y]["stats_before"]["pileup_launches"] >= 1  # the run made the pile-up
        lines = runs[y]["text"].split(b"\n")
        with_hits = np.nonzero(subj["hits"])[0]
        assert lines[-1] == b"" and len(lines) == len(with_hits) + 1 > 3
        for line, i in zip(lines[:-1], with_hits):
            c = line.split(b"\t")
            s = subj[i]
            want = [names[i].encode()] + [str(int(s[f])).encode() for f in
                                          ("length", "hits", "covered", "depth_sum", "identities_sum", "max_depth")]
            if y == "11":
                a, n = int(s["offset"]), int(s["length"])
                want.append(consensus_text(cons[a:a + n], depth[a:a + n]))
                assert len(want[-1]) == n and set(want[-1]) - set(b".-") != set()
            assert c == want, (y, i)
        for a, b in zip(runs[y]["pile"], runs["0"]["pile"]):  # the same pile-up for any -y
            assert np.array_equal(a, b)
        assert np.array_equal(runs[y]["hits"], runs["0"]["hits"])


def test_y0_y7_keep_their_bytes(fixture_runs, tmp_path):
    d, plain, runs = fixture_runs
    for y in ("0", "7"):
        assert runs[y]["text"] == plain[y] == runs[y]["text_after"], y
        assert runs[y]["stats_before"]["pileup_launches"] == 0
    assert cases.run_aln(cases.ORACLE, d, [], {}, str(tmp_path / "o.out")) == plain["0"]


def test_shards_add_up_to_the_unsharded_result(fixture_runs):
    d, plain, runs = fixture_runs
    subj, depth, ident, cons = runs["10"]["pile"]
    parts = [_run(d, ["-y", "10"], shard=(r, 3)) for r in range(3)]
    assert all(len(p["hits"]) > 0 for p in parts)
    assert np.array_equal(sum(p["pile"][1].astype(np.uint64) for p in parts), depth)
    assert np.array_equal(sum(p["pile"][2].astype(np.uint64) for p in parts), ident)
    for f in ("hits", "depth_sum", "identities_sum"):
        assert np.array_equal(sum(p["pile"][0][f].astype(np.uint64) for p in parts), subj[f]), f
    for p in parts:
        assert np.array_equal(p["pile"][0]["length"], subj["length"])
        assert np.array_equal(p["pile"][0]["offset"], subj["offset"])


def test_cli_writes_the_session_bytes(fixture_runs, tmp_path):
    d, plain, runs = fixture_runs
    for y in ("10", "11"):
        assert cases.run_aln(cases.GHOSTM, d, ["-y", y, "-D", "0"], {}, str(tmp_path / f"cli{y}.out")) == \
            runs[y]["text"]
    out2 = tmp_path / "session.out"
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", str(out2), "-D", "0", "-y", "11"]) as s:
        s.run(to_file=True)
        s.write()  # a no-op after the run wrote the file
    assert out2.read_bytes() == runs["11"]["text"]
    # ghostm search takes the styles wherever it takes -y 6 to -y 9
    out3 = tmp_path / "search.out"
    r = subprocess.run([cases.GHOSTM, "search", "-d", f"{d}/db", "-D", "0", "-y", "10", "-w", "75", f"{d}/q.fa",
                        str(out3)], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out3.read_bytes() == runs["10"]["text"]


def test_y10_needs_no_karlin_table(fixture_runs, tmp_path):
    """-G 5 has no Karlin parameters: -y 0 refuses it, -y 10 and -y 11 run like -y 1."""
    d, plain, runs = fixture_runs
    for y in ("10", "11"):
        out = tmp_path / f"g5_{y}.out"
        r = subprocess.run([cases.GHOSTM, "aln", "-i", f"{d}/q", "-d", f"{d}/db", "-o", str(out), "-D", "0", "-y", y,
                            "-G", "5"], capture_output=True)
        assert r.returncode == 0 and b"not support score option" not in r.stderr, r.stderr[-2000:]
        lines = out.read_bytes().split(b"\n")
        assert len(lines) > 3 and all(len(x.split(b"\t")) == (7 if y == "10" else 8) for x in lines[:-1])


# ------------------------------------------------------------ a replaced query set
def test_pileup_follows_a_replaced_query_set(data_root):
    d75, d24 = tx.build_fixture(data_root, 75), tx.build_fixture(data_root, 24)
    assert open(f"{d75}/db.fa").read() == open(f"{d24}/db.fa").read()
    want = {d: _run(d, []) for d in (d75, d24)}
    with Session.for_db(["-d", f"{d75}/db", "-o", os.devnull, "-D", "0"]) as s:
        for d, width in ((d75, 75), (d24, 24), (d75, 75)):
            s.set_queries_fasta(f"{d}/q.fa", width=width)
            for f in PILEUP_STATS:
                assert s.stats()[f] == 0, f
            s.run()
            assert s.hits().tobytes() == want[d]["hits"].tobytes()
            for a, b in zip(s.pileup(), want[d]["pile"]):
                assert np.array_equal(a, b)
    assert not np.array_equal(want[d75]["pile"][1], want[d24]["pile"][1])


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern, data_root):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    pr.fixture_paths(data_root, 75)  # built here, read by the child
    pr.build_tiny(data_root)
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "pileup_poison_child.py"), data_root],
                       capture_output=True, text=True, timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["hits"] == 61 + 14 + 325
