"""The read-level band pass on the device: k_band_fill<false>, k_band_walk<false>
and k_ops_compact at the stage level (BandAlignGpu against the host model, record
for record and word for word, the checker on every hit), in batches, the
refusals, the kernels under the LDS poison build; the session post-pass
(Session.hits_band) on tiled protein and DNA sets, on untiled sets, over several
chunks and shards; the -y 12 output and `ghostm search -B`."""
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
import tbext_cases as tx
import tile_cases as tc
from ghostm_amd import HIT_PATH_DTYPE, GhostmError, cigar, native, stage_band_stats
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
@pytest.mark.parametrize("name,build", bc.STAGE_CASES, ids=[n for n, _ in bc.STAGE_CASES])
def test_stage_equals_host_model(name, build):
    """All hits, one hit and no hit: the host model's bytes."""
    case = build()
    lib = native.load()
    want = case.host()
    bc.stage_setup(lib, case)
    got = {}
    for count in (None, 1, 0):
        rec, ops = got[count] = bc.gpu_band(lib, case, count=count)
        n = len(rec)
        assert np.array_equal(rec, want[0][:n]), (name, count)
        assert np.array_equal(ops, want[1][:len(ops)]) and len(ops) == int(want[0]["n_runs"][:n].sum()), (name, count)
    assert lib.FreeGpu() == 0
    case.check(*got[None])


def test_planted_indels_are_aligned_through():
    """B = 31: at least half of the hits carry a gap run and at least half have
    more than W columns (the host prototype gives 40 of 40 for both). The same
    inputs at B = 3 equal the model, with a lower score where the path would
    leave the band."""
    case = bc.indel_case(21)
    lib = native.load()
    bc.stage_setup(lib, case)
    rec, ops = bc.gpu_band(lib, case)
    rec3, ops3 = bc.gpu_band(lib, case, B=3)
    assert lib.FreeGpu() == 0
    want, want3 = case.host(), case.host(B=3)
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert np.array_equal(rec3, want3[0]) and np.array_equal(ops3, want3[1])
    strings = case.check(rec, ops)
    n = len(strings)
    assert 2 * sum(("I" in s) or ("D" in s) for s in strings) >= n
    assert 2 * sum(len(s) > bc.W for s in strings) >= n
    case.check(rec3, ops3, B=3)
    assert (rec3["score"] <= rec["score"]).all() and (rec3["score"] < rec["score"]).any()


def test_score_equals_the_unbanded_optimum_on_tiny_inputs():
    case = bc.tiny_case(31)
    lib = native.load()
    bc.stage_setup(lib, case)
    rec, ops = bc.gpu_band(lib, case)
    assert lib.FreeGpu() == 0
    case.check(rec, ops)
    M = case.M()
    for h, q in enumerate(case.sources()):
        lo, hi = int(case.s_lo[h]), int(case.s_hi[h])
        assert int(rec["score"][h]) == bc.sw_score(q, case.db[lo:hi + 1], M), h


def _rows(case, m):
    """The rows every hit's band runs (the header's formula)."""
    D = case.D.astype(np.int64)
    top = np.minimum(m - 1, case.s_hi.astype(np.int64) - D + case.B)
    bot = np.maximum(0, case.s_lo.astype(np.int64) - D - case.B)
    return np.maximum(top - bot + 1, 0)


def test_stage_in_batches():
    """GHOSTM_BAND_BATCH_HITS=7 cuts the 60 hits into nine batches and a 1 MB
    budget is honoured too (the cuts restated here from the header's formulas: a
    hit costs rows x 64 direction bytes and 2 x rows + 2B + 2 words at B = 31,
    the hits sorted by rows): the same bytes, and band_launches shows that the
    batches ran."""
    case = bc.mixed_case(6, 1500, B=31)
    lib = native.load()
    want = case.host()
    bc.stage_setup(lib, case)
    n = len(case.src)
    s0 = stage_band_stats()
    rec, ops = bc.gpu_band(lib, case)
    s1 = stage_band_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert s1["band_launches"] - s0["band_launches"] == 2  # the size call and the call with the words: one batch each
    assert s1["band_hits"] - s0["band_hits"] == 2 * n
    cells, dir_bytes = s1["band_cells"] - s0["band_cells"], s1["band_dir_bytes"] - s0["band_dir_bytes"]
    assert cells > 0 and dir_bytes * 63 == cells * 64 and s1["seconds_band"] > s0["seconds_band"]
    with _Env({"GHOSTM_BAND_BATCH_HITS": "7"}):
        rec, ops = bc.gpu_band(lib, case)
    s2 = stage_band_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    assert s2["band_launches"] - s1["band_launches"] == 2 * ((n + 6) // 7) > 10
    assert s2["band_cells"] - s1["band_cells"] == cells and s2["band_dir_bytes"] - s1["band_dir_bytes"] == dir_bytes
    assert dir_bytes == 2 * 64 * _rows(case, np.full(n, 1500)).sum()  # the size call and the call with the words
    assert lib.FreeGpu() == 0
    # the budget: 60 reads of 260-420 letters on subjects of 400, every band some 300 rows high
    case = bc.indel_case(22, n=60)
    want = case.host()
    bc.stage_setup(lib, case)
    s3 = stage_band_stats()
    with _Env({"GHOSTM_BAND_SCRATCH_MB": "1"}):
        rec, ops = bc.gpu_band(lib, case)
    s4 = stage_band_stats()
    assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
    rows = np.sort(_rows(case, np.array([len(q) for q in case.sources()])))
    cost = rows * 64 + np.where(rows > 0, 4 * (2 * rows + 2 * case.B + 2), 0)
    batches, filled = 0, None
    for c in cost:  # a batch holds at least one hit, then as many as fit the budget
        if filled is None or filled + c > (1 << 20):
            batches, filled = batches + 1, 0
        filled += int(c)
    assert batches >= 2 and s4["band_launches"] - s3["band_launches"] == 2 * batches
    assert s4["band_dir_bytes"] - s3["band_dir_bytes"] == 2 * 64 * int(rows.sum())
    assert lib.FreeGpu() == 0


def test_stage_refusals():
    """Every reason of the host test on the device entry point, the outputs
    (canary-filled) untouched; nothing is launched for a refused call."""
    case = bc.mixed_case(5, 2 * bc.W + bc.STEP + 3, B=31, n=12)
    lib = native.load()
    bc.stage_setup(lib, case)
    s0 = stage_band_stats()
    for reason, kw in bc.refusal_variants(case):
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
        rc = lib.BandAlignGpu(len(src), src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                              bc._p(case.D, ctypes.c_int32), bc._p(lo), bc._p(hi), case.W, kw.get("step", case.step),
                              kw.get("B", case.B), gaps[0], gaps[1],
                              out.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath)), bc._p(words),
                              kw.get("ops_cap", len(words)), ctypes.byref(used) if kw.get("used", True) else None)
        assert rc != 0 and reason in native.last_error(), (reason, kw, native.last_error())
        assert (out["score"] == 0xDEADBEEF).all() and (words == 0xDEADBEEF).all() and used.value == 12345, (reason, kw)
    used = ctypes.c_size_t(12345)
    rc = lib.BandAlignGpu(len(case.src), case.src.ctypes.data_as(ctypes.POINTER(native.GhostmBandSource)),
                          bc._p(case.D, ctypes.c_int32), bc._p(case.s_lo), bc._p(case.s_hi), case.W + 1, case.step, 31,
                          -11, -1, None, None, 0, ctypes.byref(used))
    assert rc != 0 and "source" in native.last_error() and used.value == 12345
    s1 = stage_band_stats()
    assert s1["band_launches"] - s0["band_launches"] == 1  # the ops_cap refusal alone ran (it knows the words only then)
    assert lib.FreeGpu() == 0


# ------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "band_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
BAND_STATS = ("seconds_band", "band_launches", "band_hits", "band_cells", "band_dir_bytes")


def fasta_records(path):
    out = []
    for block in open(path).read().split(">")[1:]:
        name, _, seq = block.partition("\n")
        out.append((name.strip(), seq.replace("\n", "")))
    return out


def back_translate(protein, r):
    by_aa = {}
    for k, aa in enumerate(tc.CODONS):
        by_aa.setdefault(aa, []).append("".join("ACGT"[(k >> s) & 3] for s in (4, 2, 0)))
    return "".join(r.choice(by_aa[a]) for a in protein)


@pytest.fixture(scope="module")
def band_reads(dataset):
    """Protein reads of up to 400 aa: cores of 60-200 residues of syn_small
    subjects, mutated, between random flanks; a third of the cores carry one
    planted indel of 1-6 letters."""
    d = dataset("syn_small")
    subjects = [x for x in fasta_records(os.path.join(d, "db.fa")) if len(x[1]) >= 150]
    r = random.Random(2025)
    reads = []
    for i in range(60):
        sub = subjects[(i * 7) % len(subjects)][1]
        a = r.randrange(0, len(sub) - 100)
        core = bc.mutate(r, sub[a:a + r.randint(60, 200)], 0.08)
        if i % 3 == 0 and len(core) > 40:
            p, k = r.randint(15, len(core) - 15), r.randint(1, 6)
            core = core[:p] + bc.rand_seq(r, k) + core[p:] if r.random() < 0.5 else core[:p] + core[p + k:]
        reads.append((f"read{i}", (bc.rand_seq(r, r.randint(0, 150)) + core + bc.rand_seq(r, r.randint(0, 120)))[:400]))
    reads.append(("short", bc.mutate(r, subjects[3][1][:90], 0.08)))
    reads.append(("random", bc.rand_seq(r, 391)))
    return reads


def dna_reads(band_reads):
    r = random.Random(9)
    reads = [(name, "ACGT"[:r.randrange(3)] + back_translate(seq, r)) for name, seq in band_reads[::2]]
    reads += [(name + "_rc", back_translate(seq, r)[::-1].translate(str.maketrans("ACGT", "TGCA")))
              for name, seq in band_reads[1:20:2]]
    return reads


def _snapshot(s, band=True):
    """What a session shows: its hits, the detail arrays, the band results, the stats."""
    out = dict(hits=s.hits(), ext=s.hits_ext(), path=s.hits_path(), rows=s.hits_rows(), stats=s.stats())
    if band:
        out["band"] = s.hits_band()
        out["stats_band"] = s.stats()
    return out


def _same_arrays(a, b):
    return (np.array_equal(a["hits"], b["hits"]) and np.array_equal(a["ext"], b["ext"])
            and all(np.array_equal(x, y) for x, y in zip(a["path"], b["path"]))
            and all(np.array_equal(x, y) for x, y in zip(a["rows"], b["rows"])))


def _tile_scores_within_band(inp, path, pops, band):
    """Per hit: whether every cell of its tile path lies within the band of its anchor."""
    return np.array([bc.within_band(bc.hit_words(path, pops, h), x[3] + int(path["q_start"][h]),
                                    x[4] + int(path["s_start"][h]), x[6], band) for h, x in enumerate(inp["per_hit"])])


@pytest.mark.parametrize("dna", [False, True], ids=["protein_tiles", "dna_tiles"])
def test_session_band_equals_host_model(dataset, band_reads, dna):
    d = dataset("syn_small")
    M = tx.blosum62()
    reads = dna_reads(band_reads) if dna else band_reads
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
        s.run()
        before = _snapshot(s, band=False)
        for f in BAND_STATS:  # nothing of the band pass runs until its results are asked for
            assert before["stats"][f] == 0, f
        rec, ops = s.hits_band()
        st1 = s.stats()
        rec2, ops2 = s.hits_band()
        st2 = s.stats()
        after = _snapshot(s)
        inp = bc.session_inputs(s, W, STEP, dna)
        path, pops = before["path"]
        # a narrower band drops the results and changes them; a refused band leaves everything
        with pytest.raises(GhostmError, match="band"):
            s.set_band(32)
        with pytest.raises(GhostmError, match="band"):
            s.set_band(0)
        assert all(np.array_equal(x, y) for x, y in zip(s.hits_band(), (rec, ops))) and s.stats() == st2
        s.set_band(3)
        rec3, ops3 = s.hits_band()
        st3 = s.stats()
        s.set_band(31)
        rec31, ops31 = s.hits_band()
        # a new query set drops them; the same set again gives them again
        s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
        assert len(s.hits_band()[0]) == 0 and len(s.hits_band()[1]) == 0
        s.run()
        for f in BAND_STATS:
            assert s.stats()[f] == 0, f
        rec_again, ops_again = s.hits_band()
    n = len(rec)
    assert n == len(before["hits"]) > (10 if dna else 30)
    want_rec, want_ops, calls = bc.session_expected(inp, W, STEP, 31, M)
    assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    strings = bc.check_session(inp, W, STEP, 31, M, rec, ops)
    # at least as good as the tile path wherever that path lies inside the band
    inside = _tile_scores_within_band(inp, path, pops, 31)
    assert inside.sum() * 10 >= 9 * n
    assert (rec["score"][inside] >= path["score"][inside]).all()
    assert sum(len(x) > W for x in strings) >= 10          # alignments no tile record could hold
    assert (rec["q_end"] > 127).any()
    # computed once and kept; the hits and the other detail arrays untouched
    assert np.array_equal(rec2, rec) and np.array_equal(ops2, ops) and st2 == st1
    assert _same_arrays(before, after)
    assert st1["band_launches"] == calls == 1 and st1["band_hits"] == n
    assert st1["seconds_band"] > 0 and st1["band_cells"] > 0 and st1["band_dir_bytes"] > 0
    # B = 3
    want3 = bc.session_expected(inp, W, STEP, 3, M)
    assert np.array_equal(rec3, want3[0]) and np.array_equal(ops3, want3[1])
    assert not np.array_equal(rec3, rec) and st3["band_launches"] == 2
    assert np.array_equal(rec31, rec) and np.array_equal(ops31, ops)
    assert np.array_equal(rec_again, rec) and np.array_equal(ops_again, ops)
    if dna:  # sources of every strand: frames 0..2 and 3..5
        frames = {int(x[2][0]) % 6 for x in inp["per_hit"] if x[2][2] > 1}
        assert frames & {0, 1, 2} and frames & {3, 4, 5}


def _untiled(d, opts, L, shard=None):
    """A file-loaded (untiled) session: its snapshot, its text and, unsharded, its inputs."""
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.devnull, "-D", "0"] + list(opts), shard=shard) as s:
        s.run()
        text = s.output()
        snap = _snapshot(s)
        snap["text"], snap["text_after"] = text, s.output()
        if shard is None:
            snap["inp"] = bc.session_inputs(s, L)
        return snap


@pytest.fixture(scope="module")
def fixture75(data_root):
    d = tx.build_fixture(data_root, 75)
    return d, {y: _untiled(d, ["-y", y] if y != "0" else [], 75) for y in ("0", "6", "7", "10", "12")}


def test_untiled_fixture_one_source_per_record(fixture75):
    """The indel fixture at L = 75, untiled: every record its own single-tile
    source of QueryLengths letters; the host model's bytes; at least the tile
    path's score for every hit."""
    d, runs = fixture75
    res = runs["0"]
    rec, ops = res["band"]
    inp = res["inp"]
    assert all(x[2][1:3] == (1, 1) and x[3] == 0 for x in inp["per_hit"]) and len(rec) > 40
    want_rec, want_ops, calls = bc.session_expected(inp, 75, None, 31, tx.blosum62())
    assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    bc.check_session(inp, 75, None, 31, tx.blosum62(), rec, ops)
    assert (rec["score"] >= res["path"][0]["score"]).all()
    for other in ("6", "7", "10", "12"):  # the same for any -y
        assert np.array_equal(runs[other]["band"][0], rec) and np.array_equal(runs[other]["band"][1], ops)


def test_two_db_chunks_one_call_per_pair(dataset):
    d = dataset("syn_chunks")  # 2 query x 3 DB chunks
    with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.devnull, "-D", "0", "-b", "1"]) as s:
        s.run()
        rec, ops = s.hits_band()
        st = s.stats()
        width = int(np.fromfile(f"{d}/q_0.inf", dtype="<u4")[1])
        inp = bc.session_inputs(s, width)
    want_rec, want_ops, calls = bc.session_expected(inp, width, None, 31, tx.blosum62())
    assert np.array_equal(rec, want_rec) and np.array_equal(ops, want_ops)
    assert calls == 6 and st["band_launches"] == 6 and st["band_hits"] == len(rec)
    bc.check_session(inp, width, None, 31, tx.blosum62(), rec, ops)


def test_three_shards_concatenate(fixture75):
    d, runs = fixture75
    whole = runs["0"]["band"]
    parts = [_untiled(d, [], 75, shard=(r, 3))["band"] for r in range(3)]
    assert all(len(p[0]) > 0 for p in parts)
    recs, at = [], 0
    for rec, ops in parts:
        r = rec.copy()
        r["ops_offset"] += at
        at += len(ops)
        recs.append(r)
    assert np.array_equal(np.concatenate(recs), whole[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])


# ------------------------------------------------------------ -y 12
LAMBDA, K = np.float32(0.267), np.float32(0.041)  # BLOSUM62 11/1 in the reference's gapped table (statistics.cpp:134-146)


def _id_text(matches, length):
    """pident as style 0 prints it: float 100 * (matches / length), %g."""
    v = np.float32(np.float32(matches) / np.float32(length)) * np.float32(100)
    return ("%g" % float(np.float32(v))).encode()


def _price(m, db_residues, score):
    """(evalue, bitscore) texts of a score for a query of m letters, in the
    formatter's float / double steps: the search space m x the database's
    residues (the reference's Statistics::CalculateSearchSpace),
    scaled = (float)space * K, E = (float)((double)scaled * exp(-1.0 * s *
    (double)lambda)), bits = ((float)s * lambda - logf(K)) / (float)log(2.0)."""
    scaled = np.float32(np.float32(np.uint64(m * db_residues)) * K)
    e = np.float32(float(scaled) * math.exp(-1.0 * score * float(LAMBDA)))
    bits = (np.float32(score) * LAMBDA - np.float32(math.log(float(K)))) / np.float32(math.log(2.0))
    return ("%g" % float(e)).encode(), ("%g" % float(np.float32(bits))).encode()


def _check_y12_lines(text12, text7, rec, ops, inp):
    """Column by column from hits_band(); a hit of read-level score 0 keeps its -y 7 line."""
    db_residues = int(sum(int(d[2].sum()) for d in inp["dbs"]))
    l12, l7 = text12.split(b"\n"), text7.split(b"\n")
    assert l12[-1] == b"" and len(l12) == len(l7) == len(rec) + 1
    small = large = 0
    for i, (a, b) in enumerate(zip(l12[:-1], l7[:-1])):
        if rec["score"][i] == 0:
            assert a == b
            continue
        c12, c7 = a.split(b"\t"), b.split(b"\t")
        assert len(c12) == 13 and c12[0:2] == c7[0:2]
        words = bc.hit_words(rec, ops, i)
        s = bc.expand(words)
        n = {c: s.count(c) for c in bc.OPS}
        gap_runs = sum(1 for w in words if int(w) & 2)
        want = [_id_text(n["="], len(s))] + [str(int(v)).encode() for v in (
            len(s), n["X"], gap_runs, rec["q_start"][i] + 1, rec["q_end"][i] + 1, rec["s_start"][i] + 1,
            rec["s_end"][i] + 1)]
        assert c12[2:10] == want, (i, c12, want)
        m = inp["per_hit"][i][2][3]
        small, large = small + (m <= 127), large + (m > 127)
        assert tuple(c12[10:12]) == _price(m, db_residues, int(rec["score"][i])), (i, m, c12)
        assert c12[12] == cigar(words).encode()
    return small, large


def test_y12_lines_on_a_tiled_set(dataset, band_reads, tmp_path):
    d = dataset("syn_small")
    out = {}
    for y in ("7", "12"):
        with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0", "-y", y]) as s:
            s.set_queries([x[1] for x in band_reads], [x[0] for x in band_reads], width=W, tile_step=STEP)
            s.run()
            out[y] = dict(text=s.output(), hits=s.hits(), stats=s.stats())
            if y == "12":
                out[y].update(band=s.hits_band(), inp=bc.session_inputs(s, W, STEP), stats_after=s.stats())
                s.set_band(3)
                s.run()
                text3, band3 = s.output(), s.hits_band()
    assert np.array_equal(out["7"]["hits"], out["12"]["hits"])  # no re-ranking, no re-merging
    assert out["7"]["stats"]["band_launches"] == 0
    assert out["12"]["stats"]["band_launches"] == 1 == out["12"]["stats_after"]["band_launches"]  # made in the run, kept
    rec, ops = out["12"]["band"]
    small, large = _check_y12_lines(out["12"]["text"], out["7"]["text"], rec, ops, out["12"]["inp"])
    assert small >= 1 and large >= 10  # queries of at most 127 letters and of more
    assert any(int(x.split(b"\t")[7]) > 127 for x in out["12"]["text"].split(b"\n")[:-1])  # qend past a record
    _check_y12_lines(text3, out["7"]["text"], band3[0], band3[1], out["12"]["inp"])
    assert text3 != out["12"]["text"]
    # the CLI writes the session's bytes
    with open(tmp_path / "reads.fa", "w") as f:
        for name, seq in band_reads:
            f.write(f">{name}\n{seq}\n")
    for band, want in (("31", out["12"]["text"]), ("3", text3)):
        r = subprocess.run([cases.GHOSTM, "search", "-w", str(W), "-T", str(STEP), "-y", "12", "-B", band, "-d",
                            os.path.join(d, "db"), str(tmp_path / "reads.fa"), str(tmp_path / f"b{band}.out")],
                           capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"b{band}.out").read_bytes() == want


@pytest.mark.parametrize("band", ["0", "32", "x", "-1", "3x"])
def test_search_cli_refuses_a_bad_band(band, tmp_path):
    """A usage error: exit 1 before any device call (the database does not even exist)."""
    r = subprocess.run([cases.GHOSTM, "search", "-y", "12", "-B", band, "-d", str(tmp_path / "nodb"),
                        str(tmp_path / "q.fa"), str(tmp_path / "out")], capture_output=True)
    assert r.returncode == 1 and not (tmp_path / "out").exists()


def test_y12_on_the_untiled_fixture(fixture75, tmp_path):
    """A line whose read-level path equals its -y 7 path is the -y 7 line byte
    for byte; the others column by column. aln -y 12 uses the default band."""
    d, runs = fixture75
    y7, y12 = runs["7"], runs["12"]
    rec, ops = y12["band"]
    path, pops = y12["path"]
    small, large = _check_y12_lines(y12["text"], y7["text"], rec, ops, y12["inp"])
    assert small > 40 and large == 0
    same = 0
    for i, (a, b) in enumerate(zip(y12["text"].split(b"\n")[:-1], y7["text"].split(b"\n")[:-1])):
        fields = ("q_start", "q_end", "s_start", "s_end", "score")
        if all(rec[f][i] == path[f][i] for f in fields) and np.array_equal(bc.hit_words(rec, ops, i),
                                                                           bc.hit_words(path, pops, i)):
            same += 1
            assert a == b, i
    assert same >= 30
    assert cases.run_aln(cases.GHOSTM, d, ["-y", "12", "-D", "0"], {}, str(tmp_path / "cli.out")) == y12["text"]


def test_other_styles_keep_their_bytes(fixture75, tmp_path):
    """-y 0, 6, 7 and 10: the same text before and after hits_band(), the same
    hits for every style, -y 0 the oracle's."""
    d, runs = fixture75
    for y in ("0", "6", "7", "10", "12"):
        assert runs[y]["text"] == runs[y]["text_after"], y
        assert np.array_equal(runs[y]["hits"], runs["0"]["hits"])
        assert runs[y]["stats"]["band_launches"] == (1 if y == "12" else 0)
    assert cases.run_aln(cases.ORACLE, d, [], {}, str(tmp_path / "o.out")) == runs["0"]["text"]
    l0, l6, l7 = (runs[y]["text"].split(b"\n") for y in ("0", "6", "7"))
    assert len(l0) == len(l6) == len(l7)
    for a, b in zip(l6[:-1], l7[:-1]):  # -y 7 shares names, evalue and bitscore with -y 6
        ca, cb = a.split(b"\t"), b.split(b"\t")
        assert ca[0:2] == cb[0:2] and ca[10:12] == cb[10:12]
