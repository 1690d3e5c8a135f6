"""The frameshift-aware read-level pass on the device: k_band_fill<true>,
k_band_walk<true> and k_ops_compact at the stage level (FrameAlignGpu against the
host model, record for record and word for word, the checker on every hit), the
lane neighbours at the band's edges, batches, the refusals, the kernels under
the LDS poison build; the session post-pass (Session.hits_frame) on tiled DNA
reads of both strands with planted single-nucleotide indels; the -y 13 output
and `ghostm search -F`."""
import ctypes
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import band_cases as bc
import cases
import frame_cases as fc
import tbext_cases as tx
from ghostm_amd import (BAND_SOURCE_DTYPE, HIT_PATH_DTYPE, GhostmError, frame_align, frame_align_host, frame_cigar,
                        native, stage_frame_stats)
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")


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
@pytest.mark.parametrize("name,build", fc.STAGE_CASES, ids=[n for n, _ in fc.STAGE_CASES])
def test_stage_equals_host_model(name, build):
    """All hits, one hit and no hit: the host model's bytes."""
    case = build()
    lib = native.load()
    want = case.host()
    fc.stage_setup(lib, case)
    got = {}
    for count in (None, 1, 0):
        rec, ops = got[count] = fc.gpu_frame(lib, case, count=count)
        n = len(rec)
        assert np.array_equal(rec, want[0][:n]), (name, count)
        assert np.array_equal(ops, want[1][:len(ops)]) and len(ops) == int(want[0]["n_runs"][:n].sum()), (name, count)
    # the Python mirror, and a shift nobody can afford
    rec, ops = frame_align(case.src, case.D, case.s_lo, case.s_hi, case.W, case.step, case.B, *case.gaps,
                           fc.NO_SHIFT)
    assert lib.FreeGpu() == 0
    want_none = case.host(shift=fc.NO_SHIFT)
    assert np.array_equal(rec, want_none[0]) and np.array_equal(ops, want_none[1])
    case.check(*got[None])


@pytest.mark.parametrize("kind,B,b", fc.LANE_CASES)
def test_stage_lane_neighbours(kind, B, b):
    """A shift at g = 0 whose source is lane b + 1, at b = 2B - 1 and at b = 2B
    (no cell; at B = 31 lane 62 is the wave's edge); a shift at g = 2 whose
    source is lane b - 1, at b = 1 and at b = 0 (no cell)."""
    case = fc.lane_edge_case(kind, B, b)
    lib = native.load()
    want = case.host()
    fc.stage_setup(lib, case)
    rec, ops = fc.gpu_frame(lib, case)
    assert lib.FreeGpu() == 0
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    s = case.check(rec, ops)[0]
    assert (("/" if kind == "early" else "\\") in s) == (0 < b < 2 * B), s


@pytest.mark.parametrize("kind", ["ins", "del"])
def test_stage_planted_truth(kind):
    case, _ = fc.truth_case(77, kind)
    lib = native.load()
    want = case.host()
    fc.stage_setup(lib, case)
    rec, ops = fc.gpu_frame(lib, case)
    assert lib.FreeGpu() == 0
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert frame_cigar(ops).count("\\" if kind == "ins" else "/") == 1


def _rows(case):
    """The nucleotide rows every hit's band runs (the header's formula)."""
    D, m = case.D.astype(np.int64), case.src["letters"].astype(np.int64)
    top = np.minimum(m - 1, case.s_hi.astype(np.int64) - D + case.B)
    bot = np.maximum(0, case.s_lo.astype(np.int64) - D - case.B)
    return 3 * np.maximum(top - bot + 1, 0)


def test_stage_in_batches():
    """A hit count that is no multiple of the waves of a block, hits of
    different row counts in one block; GHOSTM_FRAME_BATCH_HITS=1 runs every hit
    alone and a 1 MB budget cuts the sorted hits where the header's formulas say
    (rows x 64 direction bytes and rows + 4B + 4 words at B = 31): the same
    bytes, and frame_launches shows that the batches ran."""
    case = fc.many_rows_case()
    lib = native.load()
    want = case.host()
    fc.stage_setup(lib, case)
    n = len(case.src)
    assert n % 4 and len(set(_rows(case))) >= 4
    s0 = stage_frame_stats()
    rec, ops = fc.gpu_frame(lib, case)
    s1 = stage_frame_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert s1["frame_launches"] - s0["frame_launches"] == 2  # the size call and the call with the words
    assert s1["frame_hits"] - s0["frame_hits"] == 2 * n
    cells, dir_bytes = s1["frame_cells"] - s0["frame_cells"], s1["frame_dir_bytes"] - s0["frame_dir_bytes"]
    stride = (2 * case.B + 1 + 3) & ~3
    assert cells == 2 * (2 * case.B + 1) * int(_rows(case).sum()) > 0 and dir_bytes == 2 * stride * int(_rows(case).sum())
    assert s1["seconds_frame"] > s0["seconds_frame"]
    with _Env({"GHOSTM_FRAME_BATCH_HITS": "1"}):
        rec, ops = fc.gpu_frame(lib, case)
    s2 = stage_frame_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert s2["frame_launches"] - s1["frame_launches"] == 2 * n
    assert s2["frame_cells"] - s1["frame_cells"] == cells
    assert lib.FreeGpu() == 0
    # the budget: 40 strands of 200 letters a frame at B = 31
    case = fc.mixed_case(21, 200, 31, n=40)
    want = case.host()
    fc.stage_setup(lib, case)
    s3 = stage_frame_stats()
    with _Env({"GHOSTM_FRAME_SCRATCH_MB": "1"}):
        rec, ops = fc.gpu_frame(lib, case)
    s4 = stage_frame_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    rows = np.sort(_rows(case))
    cost = rows * 64 + np.where(rows > 0, 4 * (rows + 4 * case.B + 4), 0)
    batches, filled = 0, None
    for c in cost:  # a batch holds at least one hit, then as many as fit the budget
        if filled is None or filled + c > (1 << 20):
            batches, filled = batches + 1, 0
        filled += int(c)
    assert batches >= 2 and s4["frame_launches"] - s3["frame_launches"] == 2 * batches
    assert lib.FreeGpu() == 0


def test_stage_refusals():
    """Every reason of the host test on the device entry point, the outputs
    (canary-filled) untouched; nothing is launched for a refused call."""
    case = fc.mixed_case(9, 200, 31, n=12)
    lib = native.load()
    fc.stage_setup(lib, case)
    s0 = stage_frame_stats()
    seen = set()
    for reason, kw in fc.refusal_variants(case):
        if "nq" in kw:  # the resident chunk's record count is not an argument here
            continue
        src = np.ascontiguousarray(kw.get("src", case.src))
        lo = np.ascontiguousarray(kw.get("lo", case.s_lo))
        hi = np.ascontiguousarray(kw.get("hi", case.s_hi))
        gaps = kw.get("gaps", case.gaps)
        out = np.zeros(len(src), dtype=HIT_PATH_DTYPE)
        out["score"][:] = 0xDEADBEEF
        words = np.full(4096, 0xDEADBEEF, dtype=np.uint32)
        used = ctypes.c_size_t(12345)
        rc = lib.FrameAlignGpu(len(src), src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                               fc._p(case.D, ctypes.c_int32), fc._p(lo), fc._p(hi), case.W, kw.get("step", case.step),
                               kw.get("B", case.B), gaps[0], gaps[1], kw.get("shift", case.shift),
                               out.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), fc._p(words),
                               kw.get("ops_cap", len(words)), ctypes.byref(used) if kw.get("used", True) else None)
        assert rc != 0 and reason in native.last_error(), (reason, kw, native.last_error())
        assert (out["score"] == 0xDEADBEEF).all() and (words == 0xDEADBEEF).all() and used.value == 12345, (reason, kw)
        seen.add(reason)
    assert seen == {"source", "band", "bounds", "gaps", "ops_cap", "null", "shift"}
    # a strand whose frame 2 lies past the resident chunk: frame 0's record is the chunk's last
    src = case.src.copy()
    src["first_record"][0], src["tiles"][0], src["letters"][0] = case.nq - 1, 1, 100
    used = ctypes.c_size_t(12345)
    rc = lib.FrameAlignGpu(len(src), src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                           fc._p(case.D, ctypes.c_int32), fc._p(case.s_lo), fc._p(case.s_hi), case.W, case.step, 31,
                           -11, -1, -15, None, None, 0, ctypes.byref(used))
    assert rc != 0 and "source" in native.last_error() and used.value == 12345
    s1 = stage_frame_stats()
    assert s1["frame_launches"] - s0["frame_launches"] == 1  # the ops_cap refusal alone ran (it knows the words only then)
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "frame_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
FRAME_STATS = ("seconds_frame", "frame_launches", "frame_hits", "frame_cells", "frame_dir_bytes")
LAMBDA, K = np.float32(0.267), np.float32(0.041)  # BLOSUM62 11/1 in the reference's gapped table


def _revcomp(dna):
    return dna[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _inputs():
    """Six subjects of 220-330 residues and nine DNA reads of 400-900 nt: a
    stretch of a subject back-translated at a 4 % substitution rate with one or
    two single-nucleotide indels planted in it, between flanks; every other read
    reverse-complemented; n % 3 takes every value."""
    r = random.Random(20261020)
    subjects = [(f"subj{i}", fc.rand_prot(r, r.randint(220, 330))) for i in range(6)]
    reads = []
    for i in range(9):
        prot = subjects[i % 6][1]
        span = r.randint(120, 200)
        a = r.randint(0, len(prot) - span)
        core = fc.back_translate(fc.mutate(r, prot[a:a + span], 0.04))
        for _ in range(1 + i % 2):
            at = r.randint(60, len(core) - 60)
            core = core[:at] + r.choice("CG") + core[at:] if r.random() < 0.5 else core[:at] + core[at + 1:]
        n = max(len(core), r.randint(400, 900))
        n += (i - n) % 3          # n % 3 == i % 3
        left = r.randint(0, n - len(core))
        flank = fc.back_translate(fc.rand_prot(r, n // 3 + 2))
        dna = flank[:left] + core + flank[left:n - len(core)]
        assert len(dna) == n
        reads.append((f"read{i}", _revcomp(dna) if i % 2 else dna))
    return subjects, reads


def _db_fasta(tmp, subjects):
    path = os.path.join(str(tmp), "db.fa")
    with open(path, "w") as f:
        for name, seq in subjects:
            f.write(f">{name}\n{seq}\n")
    return path


def _frame_expected(s, shift=-15, band=31):
    """The host model's (records, ops, info, calls) of every hit, from the
    sources, anchors and ranges rebuilt from query_tiles(), hits_path(), the
    resolved records and the subjects' starts: the strand source begins f % 3
    records before the frame's own source."""
    inp = bc.session_inputs(s, W, STEP, dna=True)
    tiles = s.query_tiles()
    qrec = s.hits_rows()[0]["query_record"]
    per_hit = inp["per_hit"]
    want = np.zeros(len(per_hit), dtype=HIT_PATH_DTYPE)
    info, words, groups = [], [None] * len(per_hit), {}
    for h, x in enumerate(per_hit):
        groups.setdefault((x[0], x[1]), []).append(h)
        info.append(int(tiles["frame"][qrec[h]]))
    for (qi, di), idx in groups.items():
        src = np.array([(per_hit[h][2][0] - info[h] % 3,) + tuple(per_hit[h][2][1:]) for h in idx], dtype=BAND_SOURCE_DTYPE)
        lo = [per_hit[h][4] for h in idx]
        hi = [per_hit[h][4] + per_hit[h][5] - 1 for h in idx]
        rec, ops = frame_align_host(inp["chunks"][qi][2], W, inp["dbs"][di][3], tx.blosum62(), src,
                                    [per_hit[h][6] for h in idx], lo, hi, STEP, band, -11, -1, shift)
        for k, h in enumerate(idx):
            want[h] = rec[k]
            want["s_start"][h] -= lo[k]
            want["s_end"][h] -= lo[k]
            words[h] = fc.hit_words(rec, ops, k)
    at = 0
    for h in range(len(per_hit)):
        want["ops_offset"][h] = at
        at += len(words[h])
    all_ops = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, dtype=np.uint32)
    return want, all_ops, info, len(groups), inp


def _id_text(matches, length):
    v = np.float32(np.float32(matches) / np.float32(length)) * np.float32(100)
    return ("%g" % float(np.float32(v))).encode()


def _price(m, db_residues, score):
    scaled = np.float32(np.float32(np.uint64(m * db_residues)) * K)
    e = np.float32(float(scaled) * math.exp(-1.0 * score * float(LAMBDA)))
    bits = (np.float32(score) * LAMBDA - np.float32(math.log(float(K)))) / np.float32(math.log(2.0))
    return ("%g" % float(e)).encode(), ("%g" % float(np.float32(bits))).encode()


def _check_y13_lines(text13, text7, rec, ops, info, path, pops, tiles, qrec, db_residues):
    """Column by column from hits_frame() and frame_info(); a hit of frame score
    0 prints its tile path in nucleotides with the -y 7 line's E-value and bits."""
    l13, l7 = text13.split(b"\n"), text7.split(b"\n")
    assert l13[-1] == b"" and len(l13) == len(l7) == len(rec) + 1
    shifted = 0
    for i, (a, b) in enumerate(zip(l13[:-1], l7[:-1])):
        c13, c7 = a.split(b"\t"), b.split(b"\t")
        assert len(c13) == 15 and c13[0:2] == c7[0:2]
        n_nt, strand = int(info["read_nt"][i]), int(info["strand"][i])
        if rec["score"][i] > 0:
            words, x = fc.hit_words(rec, ops, i), rec[i]
            q0, q1, shifts = int(x["q_start"]), int(x["q_end"]), int(info["shifts"][i])
            price = _price(int(info["letters"][i]), db_residues, int(x["score"]))
        else:
            words, x = bc.hit_words(path, pops, i), path[i]
            t = tiles[qrec[i]]
            q0 = 3 * (int(t["offset"]) + int(x["q_start"])) + int(t["frame"]) % 3
            q1 = 3 * (int(t["offset"]) + int(x["q_end"])) + int(t["frame"]) % 3 + 2
            shifts, price = 0, tuple(c7[10:12])
        s = fc.expand(words)
        cols = sum(s.count(c) for c in "=XID")
        gap_runs = sum(1 for w in words if int(w) & 15 in (2, 3))
        want = [_id_text(s.count("="), cols)] + [str(int(v)).encode() for v in (
            cols, s.count("X"), gap_runs, n_nt - q0 if strand else q0 + 1, n_nt - q1 if strand else q1 + 1,
            x["s_start"] + 1, x["s_end"] + 1)]
        assert c13[2:10] == want, (i, c13, want)
        assert tuple(c13[10:12]) == price, (i, c13)
        assert c13[12] == frame_cigar(words).encode()
        assert c13[13] == (("-" if strand else "") + str(q0 % 3 + 1)).encode() and c13[14] == str(shifts).encode()
        assert shifts == s.count("/") + s.count("\\")
        shifted += shifts > 0
    return shifted


@pytest.fixture(scope="module")
def frame_runs(tmp_path_factory):
    """One session per style on the same database and reads; what each shows
    before and after its frame results are taken."""
    tmp = tmp_path_factory.mktemp("frame")
    subjects, reads = _inputs()
    db = _db_fasta(tmp, subjects)
    out = dict(tmp=tmp, db=db, reads=reads, subjects=subjects)
    for y in ("7", "12", "13"):
        with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y]) as s:
            s.set_db_fasta(db)
            s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W, dna=True, tile_step=STEP)
            s.run()
            r = dict(stats_before=s.frame_stats(), hits=s.hits(), text=s.output())
            if y != "13":
                r["band"] = s.hits_band()
            r["frame"] = s.hits_frame()
            r["info"] = s.frame_info()
            r["stats"] = s.frame_stats()
            r["frame_again"], r["stats_again"] = s.hits_frame(), s.frame_stats()
            r["text_after"] = s.output()
            if y != "13":
                r["band_after"] = s.hits_band()
            r["path"], r["tiles"] = s.hits_path(), s.query_tiles()
            r["qrec"] = s.hits_rows()[0]["query_record"]
            r["want"] = _frame_expected(s)
            if y == "7":
                with pytest.raises(GhostmError, match="shift"):
                    s.set_frame_shift(1)
                with pytest.raises(GhostmError, match="shift"):
                    s.set_frame_shift(-(1 << 20) - 1)
                assert s.frame_stats() == r["stats"]
                s.set_frame_shift(-3)
                r["frame3"], r["stats3"] = s.hits_frame(), s.frame_stats()
                r["want3"] = _frame_expected(s, shift=-3)
                s.set_band(3)
                r["frame_b3"] = s.hits_frame()
                r["want_b3"] = _frame_expected(s, shift=-3, band=3)
            out[y] = r
    return out


def test_session_frame_equals_host_model(frame_runs):
    r = frame_runs["7"]
    rec, ops = r["frame"]
    want_rec, want_ops, frames, calls, inp = r["want"]
    n = len(rec)
    assert n == len(r["hits"]) >= 8
    for f in FRAME_STATS:  # nothing of the frame pass runs until its results are asked for
        assert r["stats_before"][f] == 0, f
    assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    info = r["info"]
    assert [int(x) for x in info["strand"]] == [f // 3 for f in frames]
    read_nt = {name: len(seq) for name, seq in frame_runs["reads"]}
    names = [x[0] for x in frame_runs["reads"]]
    for h in range(n):
        t = r["tiles"][r["qrec"][h]]
        assert int(info["read_nt"][h]) == read_nt[names[int(t["record"])]]
        assert int(info["letters"][h]) == int(t["letters"]) == int(info["read_nt"][h]) // 3
        assert int(info["shifts"][h]) == sum(int(w) >> 4 for w in fc.hit_words(rec, ops, h) if int(w) & 15 >= 4)
    assert {int(x) % 3 for x in info["read_nt"]} == {0, 1, 2} and set(int(x) for x in info["strand"]) == {0, 1}
    # the checker on every hit, along the strand's frames read through the tile records
    M = [int(x) for x in np.asarray(tx.blosum62()).reshape(-1)]
    for h, (qi, di, src, offset, pos, length, D) in enumerate(inp["per_hit"]):
        first = src[0] - frames[h] % 3
        fr = tuple(bc.source_codes(inp["chunks"][qi][2], W, STEP, (first + g,) + tuple(src[1:])) for g in range(3))
        x = dict(q_start=rec["q_start"][h], q_end=rec["q_end"][h], s_start=int(rec["s_start"][h]) + pos,
                 s_end=int(rec["s_end"][h]) + pos, score=rec["score"][h], n_runs=rec["n_runs"][h])
        fc.check_frame_path(fr, inp["dbs"][di][3], M, x, fc.hit_words(rec, ops, h), D, 31, pos, pos + length - 1, -11, -1,
                            -15)
    # the planted indels are aligned through: shifts, and a frame score above the band score
    band = r["band"][0]
    assert (info["shifts"] >= 1).sum() >= 4
    assert (rec["score"] >= band["score"]).all() and (rec["score"] > band["score"]).sum() >= 4
    # computed once and kept
    assert all(np.array_equal(a, b) for a, b in zip(r["frame_again"], r["frame"])) and r["stats_again"] == r["stats"]
    assert r["stats"]["frame_launches"] == calls == 1 and r["stats"]["frame_hits"] == n
    assert r["stats"]["seconds_frame"] > 0 and r["stats"]["frame_cells"] > 0 and r["stats"]["frame_dir_bytes"] > 0
    # another cost, another band: dropped and made again
    assert np.array_equal(r["frame3"][0], r["want3"][0]) and np.array_equal(r["frame3"][1], r["want3"][1])
    assert not np.array_equal(r["frame3"][0], rec) and r["stats3"]["frame_launches"] == 2
    assert np.array_equal(r["frame_b3"][0], r["want_b3"][0]) and np.array_equal(r["frame_b3"][1], r["want_b3"][1])


def test_other_styles_keep_their_bytes(frame_runs):
    """The -y 7 and -y 12 text and hits_band() are the same before and after the
    frame results are taken, and every style sees the same hits."""
    for y in ("7", "12"):
        r = frame_runs[y]
        assert r["text"] == r["text_after"], y
        assert all(np.array_equal(a, b) for a, b in zip(r["band"], r["band_after"])), y
        assert np.array_equal(r["hits"], frame_runs["13"]["hits"])
        assert all(np.array_equal(a, b) for a, b in zip(r["frame"], frame_runs["13"]["frame"]))
    assert frame_runs["13"]["stats_before"]["frame_launches"] == 1 == frame_runs["13"]["stats"]["frame_launches"]


def test_y13_lines(frame_runs):
    r13, r7, r12 = frame_runs["13"], frame_runs["7"], frame_runs["12"]
    rec, ops = r13["frame"]
    db_residues = sum(len(s) for _, s in frame_runs["subjects"])
    shifted = _check_y13_lines(r13["text"], r7["text"], rec, ops, r13["info"], r13["path"][0], r13["path"][1],
                               r13["tiles"], r13["qrec"], db_residues)
    assert shifted >= 4 and r13["text"] == r13["text_after"]
    # a line with a shift whose alignment goes on past where the single frame's -y 12 line ends
    beyond = 0
    for a, b, info in zip(r13["text"].split(b"\n")[:-1], r12["text"].split(b"\n")[:-1], r13["info"]):
        c13, c12 = a.split(b"\t"), b.split(b"\t")
        if int(c13[14]) >= 1 and not info["strand"]:
            beyond += int(c13[7]) > 3 * int(c12[7]) + 2  # the frame's letter e ends at nucleotide 3e + g + 2 at most
    assert beyond >= 1
    assert any(int(x.split(b"\t")[6]) > int(x.split(b"\t")[7]) for x in r13["text"].split(b"\n")[:-1])  # a reverse strand


def test_search_cli_writes_the_session_bytes(frame_runs, tmp_path):
    with open(tmp_path / "reads.fa", "w") as f:
        for name, seq in frame_runs["reads"]:
            f.write(f">{name}\n{seq}\n")
    r = subprocess.run([cases.GHOSTM, "search", "-q", "d", "-w", str(3 * W), "-T", str(STEP), "-y", "13", "-F", "15",
                        "-f", frame_runs["db"], str(tmp_path / "reads.fa"), str(tmp_path / "y13.out")],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "y13.out").read_bytes() == frame_runs["13"]["text"]
    for bad in ("-1", "x", "1048577", "3x"):
        r = subprocess.run([cases.GHOSTM, "search", "-y", "13", "-F", bad, "-d", str(tmp_path / "nodb"),
                            str(tmp_path / "q.fa"), str(tmp_path / "out")], capture_output=True)
        assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_protein_and_untiled_sets_are_refused(frame_runs):
    reads = frame_runs["reads"]
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "13"]) as s:
        s.set_db_fasta(frame_runs["db"])
        s.set_queries([x[1][:300] for x in reads], [x[0] for x in reads], width=3 * W, dna=True)  # untiled
        with pytest.raises(GhostmError, match="tiled"):
            s.run()
        with pytest.raises(GhostmError, match="tiled"):
            s.hits_frame()
        with pytest.raises(GhostmError, match="tiled"):
            s.frame_info()
        s.set_queries([x[1] for x in frame_runs["subjects"]], [x[0] for x in frame_runs["subjects"]], width=W,
                      tile_step=STEP)  # protein tiles
        with pytest.raises(GhostmError, match="tiled"):
            s.hits_frame()
        assert s.frame_stats()["frame_launches"] == 0
