"""The read-level cull on the device: k_read_cull at the stage level (ReadCullGpu
against GhostmReadCullHost, every record equal: the small shapes, the reads at
the class borders of 64, 256 and 1024 hits and past them, one call that mixes
all classes, the largest coordinates, the batch cuts, the refusals, the LDS
poison build); the session post-pass (Session.read_cull) on a read that
carries two genes, as protein and as DNA with a planted indel, with -b 1 per
read and per tile (tile groups); -y 20 and -y 21; the setters left off change
nothing."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cases
import frame_cases as fc
import pileup_cases as pc
import readcull_cases as cc
from ghostm_amd import (CULL_DUP, CULL_KEPT, CULL_OUT_DTYPE, GhostmError, native, read_cull, read_cull_host,
                        stage_read_cull_stats)
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SHAPES = cc.shape_cases()
_Env = pc.pr_env


def _counted(case, want):
    """ReadCullGpu on the case, the counters checked against the records"""
    s0 = stage_read_cull_stats()
    got = read_cull(*case)
    s1 = stage_read_cull_stats()
    rb = case[0]
    inside = want[int(rb[0]):int(rb[-1])]["status"]
    assert s1["cull_hits"] - s0["cull_hits"] == len(inside)
    assert s1["cull_reads"] - s0["cull_reads"] == int((np.diff(rb.astype(np.int64)) > 0).sum())
    for k, name in enumerate(("cull_kept", "cull_dups", "cull_culled")):
        assert s1[name] - s0[name] == int((inside == k).sum()), name
    assert (s1["cull_launches"] > s0["cull_launches"]) == (len(inside) > 0)
    return got, s1["cull_launches"] - s0["cull_launches"]


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_equals_host_model_on_the_shapes(name):
    case = SHAPES[name]
    want = read_cull_host(*case)
    cc.expected_shapes(name, want)
    got, _ = _counted(case, want)
    cc.assert_same(got, want, name)


@pytest.mark.parametrize("n", cc.SIZES)
def test_stage_equals_host_model_at_the_class_borders(n):
    case = cc.sized_read(n)
    want = read_cull_host(*case)
    got, launches = _counted(case, want)
    cc.assert_same(got, want, n)
    assert launches == 1


def test_stage_mixed_classes_and_batch_cuts():
    """One call with reads of every class and reads without hits; then the same
    call in batches of three reads, and in batches cut by the byte budget at
    every read above the LDS classes: the records do not depend on the cuts."""
    case = cc.mixed_call()
    want = read_cull_host(*case)
    got, launches = _counted(case, want)
    cc.assert_same(got, want, "one batch")
    assert launches == 1
    nreads = len(case[0]) - 1
    with _Env({"GHOSTM_CULL_BATCH_READS": "3"}):
        got, launches = _counted(case, want)
    cc.assert_same(got, want, "batches of three reads")
    sizes = np.diff(case[0].astype(np.int64))
    assert launches == sum(1 for b in range(0, nreads, 3) if sizes[b:b + 3].sum() > 0) > 3
    # ten reads of 1025 hits: 40 bytes a hit and a table of 13 * 2048 words, 147,504 bytes a read with
    # its list entry, so a budget of one megabyte takes seven reads and then three
    big = cc.join([cc.sized_read(1025, seed=s) for s in range(10)], 1, 50)
    big_want = read_cull_host(*big)
    with _Env({"GHOSTM_CULL_SCRATCH_MB": "1"}):
        got, cuts = _counted(big, big_want)
    cc.assert_same(got, big_want, "batches of a megabyte")
    assert cuts == 2
    cc.assert_same(read_cull(*big), big_want, "the ten in one batch")
    # a second call reuses the buffers and gives the same records
    cc.assert_same(read_cull(*case), want, "again")
    # hits outside every read keep the caller's bytes
    _, h, k, pct = SHAPES["nested"]
    out = np.full(4 * len(h), 0x5A5A5A5A, dtype=np.uint32).view(CULL_OUT_DTYPE)
    rb = np.array([1, 3], dtype=np.uint32)
    read_cull(rb, h, k, pct, out=out)
    assert out[0].tolist() == (0x5A5A5A5A,) * 4
    cc.assert_same(out[1:], read_cull_host(rb, h, k, pct)[1:], "inner read")
    assert native.load().FreeGpu() == 0


def test_stage_random_reads():
    """the host test's random reads, joined into three calls"""
    calls = cc.random_calls(150)
    for top_k, pct in ((1, 50), (2, 30), (255, 100)):
        case = cc.join(calls, top_k, pct)
        cc.assert_same(read_cull(*case), read_cull_host(*case), ("random", top_k, pct))


def test_stage_refusals():
    """Every reason on the device entry point, the outputs untouched; no refused
    call launches anything."""
    read_cull(*SHAPES["one_hit"])   # the device module exists
    s0 = stage_read_cull_stats()
    cc.check_refusals("ReadCullGpu")
    assert stage_read_cull_stats() == s0
    with pytest.raises(GhostmError, match="param"):
        read_cull(*SHAPES["nested"][:2], cover_pct=101)


@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "readcull_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
A, B, C = 0, 1, 2   # the subjects' db_ids


def _inputs():
    """Three subjects of 150 residues and one read of about 400 letters: gene A
    at a 3 % substitution rate, a linker of 30 letters, gene B diverged at 12 %,
    70 letters of noise. The same read as DNA: back-translated, with one
    nucleotide planted in the middle of gene A."""
    r = random.Random(20261122)
    subjects = [(name, fc.rand_prot(r, 150)) for name in ("geneA", "geneB", "geneC")]
    prot = fc.mutate(r, subjects[A][1], 0.03) + fc.rand_prot(r, 30) + fc.mutate(r, subjects[B][1], 0.12) + fc.rand_prot(r, 70)
    dna = fc.back_translate(prot)
    dna = dna[:3 * 75 + 1] + "G" + dna[3 * 75 + 1:]
    return subjects, [("read0", prot)], [("read0", dna)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("readcull"))
    subjects, prot, dna = _inputs()
    out = dict(tmp=tmp, db=os.path.join(tmp, "db.fa"), prot=prot, dna=dna, prot_fa=os.path.join(tmp, "prot.fa"),
               dna_fa=os.path.join(tmp, "dna.fa"))
    for path, records in ((out["db"], subjects), (out["prot_fa"], prot), (out["dna_fa"], dna)):
        with open(path, "w") as f:
            for name, seq in records:
                f.write(f">{name}\n{seq}\n")
    return out


def _open(files, dna, y="0", groups=None, cull=None):
    s = Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y, "-b", "1"])
    s.set_db_fasta(files["db"])
    if groups is not None:
        s.set_tile_groups(groups)
    if cull is not None:
        s.set_cull(*cull)
    reads = files["dna" if dna else "prot"]
    s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
    return s


def _session_model(s, frame, dna, top_k=1, cover_pct=50):
    """GhostmReadCullHost on the records the contract names, made here from the
    session's hits, paths and tile table."""
    hits, tiles = s.hits(), s.query_tiles()
    band = s.hits_band()[0]
    t = tiles[s.hits_band_rows()[0]["query_record"]]   # a record of the hit's source: its read and its frame
    path = s.hits_frame()[0] if frame else band
    n = len(hits)
    begin = [0] + [h for h in range(1, n) if t["record"][h] != t["record"][h - 1]] + [n]
    rec = np.zeros(n, dtype=cc.CULL_HIT_DTYPE)
    rec["subject"], rec["score"] = hits["db_id"], path["score"]
    info = s.frame_info() if dna else None
    for h in range(n):
        if not path["score"][h]:
            continue
        q0, q1 = int(path["q_start"][h]), int(path["q_end"][h])
        if dna:
            g, strand, nt = int(t["frame"][h]) % 3, int(info["strand"][h]), int(info["read_nt"][h])
            assert strand == int(t["frame"][h]) // 3
            p0, p1 = (q0, q1) if frame else (3 * q0 + g, 3 * q1 + g + 2)
            q0, q1 = sorted((nt - 1 - p0, nt - 1 - p1) if strand else (p0, p1))
        rec[h] = (hits["db_id"][h], path["score"][h], q0, q1, path["s_start"][h], path["s_end"][h])
    return read_cull_host(np.array(begin, dtype=np.uint32), rec, top_k, cover_pct)


def _kept_subjects(s, out):
    return sorted(s.hits()["db_id"][out["status"] == CULL_KEPT].tolist())


def _check_dups(s, out):
    """every DUP names a KEPT hit of its subject that ranks before it"""
    hits = s.hits()
    dups = np.flatnonzero(out["status"] == CULL_DUP)
    for h in dups:
        k = int(out["detail"][h])
        assert out["status"][k] == CULL_KEPT and hits["db_id"][k] == hits["db_id"][h] and out["order"][k] < out["order"][h]
    return len(dups)


def _want_text(lines, out):
    kept = sorted(np.flatnonzero(out["status"] == CULL_KEPT), key=lambda h: out["kept_rank"][h])   # one read
    return b"".join(lines[h] + b"\t%d\t%d\n" % (out["kept_rank"][h], out["detail"][h]) for h in kept)


def test_session_protein_two_genes(files, tmp_path):
    with _open(files, False, groups=False) as s:   # -b 1 per read: the better-conserved gene only
        s.run()
        assert s.read_cull_stats()["cull_launches"] == 0
        out = s.read_cull()
        assert len(out) == 1 and _kept_subjects(s, out) == [A]
        assert s.read_cull_stats()["cull_launches"] == 1 and s.read_cull_stats()["cull_kept"] == 1
    with _open(files, False, y="12", groups=True) as s:   # -b 1 per tile
        s.run()
        lines = s.output().splitlines()
        assert s.read_cull_stats()["cull_launches"] == 0   # -y 12 asks for no cull
        out = s.read_cull()
        st = s.read_cull_stats()
        assert st["cull_launches"] == 1 and st["cull_reads"] == 1 and st["cull_hits"] == len(out) == len(lines) >= 4
        cc.assert_same(out, _session_model(s, False, False), "protein")
        kept = _kept_subjects(s, out)
        assert kept.count(A) == 1 and kept.count(B) == 1, kept
        # adjacent tiles found gene A on one diagonal: the second is the first again
        assert _check_dups(s, out) >= 1 and (s.hits()["db_id"][out["status"] == CULL_DUP] == A).any()
        assert s.read_cull() is not out and s.read_cull_stats() == st   # kept: the second call launches nothing
        s.set_cull(1, 50)   # no change
        s.read_cull()
        assert s.read_cull_stats() == st
        s.set_cull(2, 100)   # a change drops the result
        cc.assert_same(s.read_cull(), _session_model(s, False, False, 2, 100), "protein, 2 / 100")
        assert s.read_cull_stats()["cull_launches"] == 2
        with pytest.raises(GhostmError, match="param"):
            s.set_cull(0, 50)
        with pytest.raises(GhostmError, match="tiled"):   # refused where hits_frame() is
            s.read_cull(True)
        want = _want_text(lines, out)
    with _open(files, False, y="20", groups=True) as s:
        s.run()
        assert s.output() == want and want.count(b"\n") >= 2
        assert s.read_cull_stats()["cull_launches"] == 1
    out_path = str(tmp_path / "y20.out")   # the command form: -g, and -K -C at their defaults
    cmd = [cases.GHOSTM, "search", "-q", "p", "-w", str(W), "-T", str(STEP), "-y", "20", "-b", "1", "-D", "0", "-g",
           "-K", "1", "-C", "50", "-f", files["db"], files["prot_fa"], out_path]
    r = subprocess.run(cmd, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out_path, "rb").read() == want


def test_session_dna_two_genes(files):
    with _open(files, True, groups=False) as s:
        s.run()
        out = s.read_cull(True)
        # one gene only; which one the tile scores decide (the indel halves gene A's tiles)
        assert len(out) == 1 and _kept_subjects(s, out) in ([A], [B])
    with _open(files, True, y="13", groups=True) as s:
        s.run()
        lines13 = s.output().splitlines()
        assert s.read_cull_stats()["cull_launches"] == 0
        frame = s.read_cull(True)
        cc.assert_same(frame, _session_model(s, True, True), "dna, frame paths")
        band = s.read_cull(False)
        cc.assert_same(band, _session_model(s, False, True), "dna, band paths")
        assert s.read_cull_stats()["cull_launches"] == 2
        assert int(s.frame_info()["shifts"].sum()) > 0   # the planted nucleotide
        kept = _kept_subjects(s, frame)
        assert kept.count(A) == 1 and kept.count(B) == 1, kept   # the frame path crosses the indel: one alignment of A
        assert _check_dups(s, frame) >= 1
        assert {A, B} <= set(_kept_subjects(s, band))
        _check_dups(s, band)
        want21 = _want_text(lines13, frame)
    with _open(files, True, y="21", groups=True) as s:
        s.run()
        assert s.output() == want21 and want21.count(b"\n") >= 2
    with _open(files, True, y="12", groups=True) as s:
        s.run()
        want20 = _want_text(s.output().splitlines(), band)
    with _open(files, True, y="20", groups=True) as s:
        s.run()
        assert s.output() == want20


def test_setters_off_change_nothing(files):
    """Tile groups switched on and off again and other cull parameters, but no
    cull call: the -y 12 bytes and the hits of a session that never touched the
    new setters."""
    with _open(files, False, y="12") as s:
        s.run()
        plain, plain_hits = s.output(), s.hits()
    with _open(files, False, y="12", groups=True) as s:
        s.set_tile_groups(False)
        s.set_cull(3, 10)
        s.set_queries([x[1] for x in files["prot"]], [x[0] for x in files["prot"]], width=W, tile_step=STEP)
        s.run()
        assert s.output() == plain and np.array_equal(s.hits(), plain_hits)
        assert s.read_cull_stats()["cull_launches"] == 0
