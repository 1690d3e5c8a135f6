"""The read-level aligned rows on the device: k_read_rows at the stage level
(ReadRowsGpu against the host model, records and rows byte for byte: hand-made
band and frame paths on both strand layouts, the passes' own paths with the
rescore equal to the score, batches, the refusals, the LDS poison build); the
session post-passes (Session.hits_band_rows, hits_frame_rows) on tiled DNA
reads of both strands with planted single-nucleotide indels; the -y 14 and
-y 15 text."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import band_cases as bc
import frame_cases as fc
import readrows_cases as rc
import tbext_cases as tx
from ghostm_amd import (BAND_SOURCE_DTYPE, READ_ROWS_DTYPE, GhostmError, native, read_rows, read_rows_host, rows_of,
                        stage_read_rows_stats)
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SETS = rc.stage_sets()


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
@pytest.mark.parametrize("name,build", SETS, ids=[n for n, _ in SETS])
def test_stage_equals_host_model(name, build):
    """All hits, one hit, no hit, and the counts alone (rows == NULL)."""
    rs = build()
    want = rs.host()
    lib = native.load()
    rc.stage_setup(lib, rs)
    rec, rows = rc.gpu_rows(lib, rs)
    assert np.array_equal(rec, want[0]) and bytes(rows) == bytes(want[1])
    if not name.startswith("hand"):  # a path the passes made: the rows prove the DP's score
        assert (rec["rescore"] == rs.rec["score"].astype(np.int64)).all() and (rs.rec["score"] > 0).any()
    one, one_rows = rc.gpu_rows(lib, rs, count=1)
    assert np.array_equal(one, want[0][:1]) and bytes(one_rows) == bytes(want[1][:3 * int(want[0]["columns"][0])])
    none, none_rows = rc.gpu_rows(lib, rs, count=0)
    assert len(none) == 0 and len(none_rows) == 0
    counts, _ = rc.gpu_rows(lib, rs, rows=False)
    assert np.array_equal(counts, want[0])
    got = read_rows(rs.src, rs.rec, rs.ops, rs.W, rs.step, rs.frame, *rs.gaps, rs.shift)   # the Python wrapper
    assert np.array_equal(got[0], want[0]) and bytes(got[1]) == bytes(want[1])
    assert lib.FreeGpu() == 0


def _long_set():
    """12 hits of 30 to 50 thousand columns each (a pair, then one long 'D' run):
    1.4 MB of rows, so that a 1 MB budget cuts them."""
    rnd = random.Random(4301)
    qseq, src = bc.tile_records([bc.rand_seq(rnd, 200)], rc.W, rc.STEP, 1)
    db = np.array([rc.END] + [rnd.randrange(20) for _ in range(60000)] + [rc.END], dtype=np.uint8)
    paths = [(h, 1 + 7 * h, [2 << 4 | 0, (30000 + 1777 * h) << 4 | 3, 1 << 4 | 1]) for h in range(12)]
    rec, ops = rc._paths(paths)
    return rc.RowSet(qseq, rc.W, rc.STEP, db, tx.blosum62(), [src[0]] * 12, rec, ops, 0)


def test_stage_in_batches():
    """A hit count that is no multiple of the waves of a block;
    GHOSTM_READ_ROWS_BATCH_HITS=1 runs every hit alone and a 1 MB budget cuts the
    hits, in hit order, where 3 bytes a column say: the same bytes, and
    read_rows_launches shows that the batches ran. The size call launches
    nothing."""
    rs = rc.hand_frame_set(1)
    lib = native.load()
    want = rs.host()
    rc.stage_setup(lib, rs)
    n = len(rs.src)
    assert n % 4
    s0 = stage_read_rows_stats()
    rec, rows = rc.gpu_rows(lib, rs)
    s1 = stage_read_rows_stats()
    assert np.array_equal(rec, want[0]) and bytes(rows) == bytes(want[1])
    assert s1["read_rows_launches"] - s0["read_rows_launches"] == 1
    assert s1["read_rows_hits"] - s0["read_rows_hits"] == n
    assert s1["read_rows_columns"] - s0["read_rows_columns"] == int(want[0]["columns"].sum())
    assert s1["seconds_read_rows"] > s0["seconds_read_rows"]
    with _Env({"GHOSTM_READ_ROWS_BATCH_HITS": "1"}):
        rec, rows = rc.gpu_rows(lib, rs)
    s2 = stage_read_rows_stats()
    assert np.array_equal(rec, want[0]) and bytes(rows) == bytes(want[1])
    assert s2["read_rows_launches"] - s1["read_rows_launches"] == n
    assert lib.FreeGpu() == 0
    rs = _long_set()
    want = rs.host()
    rc.stage_setup(lib, rs)
    s3 = stage_read_rows_stats()
    with _Env({"GHOSTM_READ_ROWS_SCRATCH_MB": "1"}):
        rec, rows = rc.gpu_rows(lib, rs)
    s4 = stage_read_rows_stats()
    assert np.array_equal(rec, want[0]) and bytes(rows) == bytes(want[1])
    batches, filled = 0, None
    for c in 3 * want[0]["columns"].astype(np.int64):  # a batch holds at least one hit, then as many as fit the budget
        if filled is None or filled + c > (1 << 20):
            batches, filled = batches + 1, 0
        filled += int(c)
    assert batches >= 2 and s4["read_rows_launches"] - s3["read_rows_launches"] == batches
    assert lib.FreeGpu() == 0


@pytest.mark.parametrize("build", [rc.hand_band_set, lambda: rc.hand_frame_set(0)], ids=["band", "frame"])
def test_stage_refusals(build):
    """Every reason of the host test on the device entry point, the outputs
    (canary-filled) untouched; no refused call launches a kernel."""
    rs = build()
    lib = native.load()
    rc.stage_setup(lib, rs)
    s0 = stage_read_rows_stats()
    seen = set()
    variants = [(r, kw) for r, kw in rc.refusal_variants(rs) if "nq" not in kw]  # nq is no argument here
    for reason, kw in variants + [("source", dict(W=rs.W - 1))]:
        src = np.ascontiguousarray(kw.get("src", rs.src))
        rec = np.ascontiguousarray(kw.get("rec", rs.rec))
        ops = np.ascontiguousarray(kw.get("ops", rs.ops))
        out = np.zeros(len(src), dtype=READ_ROWS_DTYPE)
        out["columns"][:] = 0xDEADBEEF
        rows = np.full(1 << 14, 0xA7, dtype=np.uint8)
        used = ctypes.c_size_t(12345)
        code = lib.ReadRowsGpu(len(src), None if kw.get("null_src") else
                               src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                               rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), rc._p(ops), len(ops),
                               kw.get("W", rs.W), kw.get("step", rs.step), rs.frame, rs.gaps[0], rs.gaps[1],
                               kw.get("shift", rs.shift), out.ctypes.data_as(ctypes.POINTER(native.GhostmHitReadRows)),
                               rc._p(rows, ctypes.c_uint8), kw.get("rows_cap", len(rows)), ctypes.byref(used))
        assert code != 0 and reason in native.last_error(), (reason, kw, native.last_error())
        assert (out["columns"] == 0xDEADBEEF).all() and (rows == 0xA7).all() and used.value == 12345, (reason, kw)
        seen.add(reason)
    assert seen == {"source", "ops", "word", "bounds", "rows_cap", "null"} | ({"shift"} if rs.frame else set())
    if rs.frame:  # a strand whose frame 2 lies past the resident chunk: frame 0's record is the chunk's last
        src = rs.src.copy()
        src["first_record"][0], src["tiles"][0], src["letters"][0] = rs.nq - 1, 1, 100
        used = ctypes.c_size_t(12345)
        code = lib.ReadRowsGpu(len(src), src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                               rs.rec.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), rc._p(rs.ops), len(rs.ops),
                               rs.W, rs.step, 1, -11, -1, -15, None, None, 0, ctypes.byref(used))
        assert code != 0 and "source" in native.last_error() and used.value == 12345
    assert stage_read_rows_stats()["read_rows_launches"] == s0["read_rows_launches"]
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "readrows_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
STATS = ("seconds_read_rows", "read_rows_launches", "read_rows_hits", "read_rows_columns")


def _revcomp(dna):
    return dna[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _inputs():
    """Four subjects of 220-330 residues and six DNA reads of 500-800 nt: a
    stretch of a subject back-translated at a 4 % substitution rate with one
    single-nucleotide indel planted in its middle, between flanks; every other
    read reverse-complemented."""
    r = random.Random(20261021)
    subjects = [(f"subj{i}", fc.rand_prot(r, r.randint(220, 330))) for i in range(4)]
    reads = []
    for i in range(6):
        prot = subjects[i % 4][1]
        span = r.randint(120, 200)
        a = r.randint(0, len(prot) - span)
        core = fc.back_translate(fc.mutate(r, prot[a:a + span], 0.04))
        at = r.randint(len(core) // 2 - 30, len(core) // 2 + 30)
        core = core[:at] + r.choice("CG") + core[at:] if i % 3 else core[:at] + core[at + 1:]
        n = max(len(core), r.randint(500, 800))
        left = r.randint(0, n - len(core))
        flank = fc.back_translate(fc.rand_prot(r, n // 3 + 2))
        dna = flank[:left] + core + flank[left:n - len(core)]
        assert len(dna) == n
        reads.append((f"read{i}", _revcomp(dna) if i % 2 else dna))
    return subjects, reads


def _expected_rows(s, frame, path, ops):
    """The host model's records and bytes of every hit's read-level path, from
    the sources rebuilt from what the session shows (band_cases.session_inputs):
    one call per (query chunk, DB chunk), the bytes in hit order, query_record
    global."""
    inp = bc.session_inputs(s, W, STEP, dna=True)
    tiles, qrec = s.query_tiles(), s.hits_rows()[0]["query_record"]
    per_hit = inp["per_hit"]
    want = np.zeros(len(per_hit), dtype=READ_ROWS_DTYPE)
    text = [b""] * len(per_hit)
    groups = {}
    for h, x in enumerate(per_hit):
        groups.setdefault((x[0], x[1]), []).append(h)
    for (qi, di), idx in groups.items():
        back = [int(tiles["frame"][qrec[h]]) % 3 if frame else 0 for h in idx]
        src = np.array([(per_hit[h][2][0] - b,) + tuple(per_hit[h][2][1:]) for h, b in zip(idx, back)], dtype=BAND_SOURCE_DTYPE)
        rec = path[idx].copy()
        for k, h in enumerate(idx):
            rec["s_start"][k] += per_hit[h][4]
        got, rows = read_rows_host(inp["chunks"][qi][2], W, inp["dbs"][di][3], tx.blosum62(), src, rec, ops, STEP, frame,
                                   -11, -1, -15)
        for k, h in enumerate(idx):
            want[h] = got[k]
            want["query_record"][h] += inp["chunks"][qi][0]
            text[h] = b"".join(rows_of(got, rows, k))
    at = 0
    for h in range(len(per_hit)):
        want["rows_offset"][h] = at
        at += len(text[h])
    return want, b"".join(text), len(groups)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One session per style on the same database and reads."""
    tmp = tmp_path_factory.mktemp("readrows")
    subjects, reads = _inputs()
    db = os.path.join(str(tmp), "db.fa")
    with open(db, "w") as f:
        for name, seq in subjects:
            f.write(f">{name}\n{seq}\n")
    out = dict(db=db, reads=reads, subjects=subjects)
    for y in ("0", "12", "13", "14", "15"):
        with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y]) as s:
            s.set_db_fasta(db)
            s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W, dna=True, tile_step=STEP)
            s.run()
            r = dict(text=s.output(), stats_run=s.read_rows_stats(), hits=s.hits())
            if y in ("14", "15"):
                frame = y == "15"
                r["path"] = s.hits_frame() if frame else s.hits_band()
                r["rows"] = s.hits_frame_rows() if frame else s.hits_band_rows()
                r["stats"] = s.read_rows_stats()
                r["other"] = s.hits_band_rows() if frame else s.hits_frame_rows()
                r["other_path"] = s.hits_band() if frame else s.hits_frame()
                r["stats_both"] = s.read_rows_stats()
                r["again"] = s.hits_frame_rows() if frame else s.hits_band_rows()
                r["stats_again"] = s.read_rows_stats()
                r["tile_rows"] = s.hits_rows()
                r["info"] = s.frame_info()
                r["want"] = _expected_rows(s, frame, *r["path"])
                r["want_other"] = _expected_rows(s, not frame, *r["other_path"])
                r["text_after"] = s.output()
            out[y] = r
    return out


def test_default_path_launches_nothing(runs):
    for y in ("0", "12", "13"):
        for f in STATS:
            assert runs[y]["stats_run"][f] == 0, (y, f)


@pytest.mark.parametrize("y", ["14", "15"])
def test_session_rows_equal_host_model(runs, y):
    r = runs[y]
    rec, rows = r["rows"]
    want, text, calls = r["want"]
    n = len(rec)
    assert n == len(r["hits"]) >= 6
    assert np.array_equal(rec, want) and bytes(rows) == text
    assert (rec["rescore"] == r["path"][0]["score"].astype(np.int64)).all() and (rec["rescore"] > 0).any()
    # made by the run for the text, once: one call per chunk pair
    assert r["stats_run"] == r["stats"] and r["stats"]["read_rows_launches"] == calls == 1
    assert r["stats"]["read_rows_hits"] == n and r["stats"]["read_rows_columns"] == int(rec["columns"].sum())
    assert r["stats"]["seconds_read_rows"] > 0
    # the other kind on the same session, and both kept
    other, other_rows = r["other"]
    assert np.array_equal(other, r["want_other"][0]) and bytes(other_rows) == r["want_other"][1]
    assert r["stats_both"]["read_rows_launches"] == 2
    assert np.array_equal(r["again"][0], rec) and np.array_equal(r["again"][1], rows)
    assert r["stats_again"] == r["stats_both"] and r["text"] == r["text_after"]


@pytest.mark.parametrize("y,base", [("14", "12"), ("15", "13")])
def test_y14_y15_lines(runs, y, base):
    r = runs[y]
    rec, rows = r["rows"]
    tile_rec, tile_rows = r["tile_rows"]
    level = r["path"][0]
    lines, base_lines = r["text"].split(b"\n")[:-1], runs[base]["text"].split(b"\n")[:-1]
    assert len(lines) == len(base_lines) == len(rec)
    shifted = 0
    for h, (line, head) in enumerate(zip(lines, base_lines)):
        assert line.startswith(head + b"\t"), h
        tail = line[len(head) + 1:].split(b"\t")
        assert len(tail) == 3
        src_rec, src_rows = (rec, rows) if int(level["score"][h]) > 0 else (tile_rec, tile_rows)
        q, _, s = rows_of(src_rec, src_rows, h)
        assert tail == [str(int(src_rec["positives"][h])).encode(), q, s], h
        marks = q.count(b"\\") + q.count(b"/")
        if y == "15":
            assert marks == (int(r["info"]["shifts"][h]) if int(level["score"][h]) > 0 else 0)
            assert int(head.split(b"\t")[3]) == len(q) - marks   # -y 13's length: a shift is no alignment column
            shifted += marks == 1
        else:
            assert marks == 0
    if y == "15":  # every read carries one planted indel: its hit is aligned through it with one shift
        assert shifted >= 4


def test_y15_needs_a_tiled_dna_set(runs):
    subjects = runs["subjects"]
    for y in ("13", "15"):
        with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y]) as s:
            s.set_db_fasta(runs["db"])
            s.set_queries([x[1] for x in subjects], [x[0] for x in subjects], width=W, tile_step=STEP)  # protein tiles
            with pytest.raises(GhostmError, match="tiled"):
                s.run()
            with pytest.raises(GhostmError, match="tiled"):
                s.hits_frame_rows()
            assert s.read_rows_stats()["read_rows_launches"] == 0
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "14"]) as s:   # the band rows need no DNA
        s.set_db_fasta(runs["db"])
        s.set_queries([x[1] for x in subjects], [x[0] for x in subjects], width=W, tile_step=STEP)
        s.run()
        rec, rows = s.hits_band_rows()
        assert len(rec) == len(s.hits()) >= len(subjects)
        assert (rec["rescore"] == s.hits_band()[0]["score"].astype(np.int64)).all() and (rec["shifts"] == 0).all()
        assert len(s.output().split(b"\n")) == len(rec) + 1
