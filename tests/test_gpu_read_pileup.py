"""The read-level subject pile-up on the device: k_read_pileup and
k_pileup_finish<true> at the stage level (ReadPileupGpu against the host model
and the Python model, every array equal: band and frame paths, the tile-edge
shapes at tiles of 32 positions, several windows, the refusals, the LDS
poison build); the session post-pass (Session.read_pileup,
read_subject_profile) on tiled DNA reads of both strands with planted
single-nucleotide indels and on protein reads of about 300 letters; the point of
the feature (a long read covers more than one tile's 127 positions); -y 16 to
-y 19 through `ghostm search`; two shards that add up."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import band_cases as bc
import cases
import frame_cases as fc
import pileup_cases as pc
import readpileup_cases as rp
import readrows_cases as rc
import tbext_cases as tx
from ghostm_amd import GhostmError, consensus_text, native, read_pileup, stage_read_pileup_stats
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SETS = rp.stage_sets()
STATS = ("seconds_read_pileup", "read_pileup_launches", "read_pileup_windows", "read_pileup_parts",
         "read_pileup_columns", "read_pileup_shifts")
TILE_STATS = ("seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns")
_Env = pc.pr_env


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("name,build", SETS, ids=[n for n, _ in SETS])
def test_stage_equals_host_model(name, build):
    """All hits, one hit, no hit; with the profile and with NULL, with shifts and
    with NULL; the counters count what the words say."""
    rs = build()
    lib = native.load()
    rc.stage_setup(lib, rs)
    host, gpu = rp.host_call(lib, rs), rp.gpu_call(lib)
    for count in (None, 1, 0):
        want = rp.pileup_via(host, rs, count)
        rp.assert_same(want, rp.model(rs, count), ("host", name, count))
        s0 = stage_read_pileup_stats()
        rp.check_against_model(gpu, rs, ("gpu", name, count), count, want=want)
        s1 = stage_read_pileup_stats()
        n = len(rs.src) if count is None else count
        cols, shifts = rp.charged_columns(rs.rec[:n], rs.ops)
        assert s1["read_pileup_columns"] - s0["read_pileup_columns"] == 4 * cols == 4 * int(want[0].sum())
        assert s1["read_pileup_shifts"] - s0["read_pileup_shifts"] == 4 * shifts == 4 * int(want[3].sum())
        assert s1["read_pileup_windows"] - s0["read_pileup_windows"] == 4
        assert (s1["read_pileup_launches"] > s0["read_pileup_launches"]) == (cols + shifts > 0)
    got = read_pileup(rs.src, rs.rec, rs.ops, rs.W, rs.step, len(rs.db), rs.frame, profile=True)   # the Python wrapper
    rp.assert_same(got, rp.model(rs), "wrapper")
    assert lib.FreeGpu() == 0


@pytest.mark.parametrize("strand", [0, 1])
def test_stage_tile_edges(strand):
    """Tiles of 32 positions and parts of 7 hits: the shapes of
    readpileup_cases.edge_sets, each against the Python model; the reversed
    order gives the same arrays."""
    lib = native.load()
    sets = rp.edge_sets(strand)
    first = next(iter(sets.values()))
    rc.stage_setup(lib, first)   # every set shares the query chunk and the DB chunk
    gpu = rp.gpu_call(lib)
    results = {}
    with _Env(rp.EDGE_ENV):
        for name, rs in sets.items():
            assert rs.qseq is first.qseq or np.array_equal(rs.qseq, first.qseq)
            assert np.array_equal(rs.db, first.db)
            want = rp.model(rs)
            rp.expected_edges(name, want)
            s0 = stage_read_pileup_stats()
            got = rp.pileup_via(gpu, rs)
            s1 = stage_read_pileup_stats()
            rp.assert_same(got, want, name)
            results[name] = got
            if name.endswith("copies_300"):   # 300 hits on one tile: 43 parts of at most 7
                assert s1["read_pileup_parts"] - s0["read_pileup_parts"] == 43
            if name.endswith("four_tiles"):   # one hit walked by the six tiles it meets
                assert s1["read_pileup_parts"] - s0["read_pileup_parts"] == 6
        for mode in ("frame", "band"):
            rp.assert_same(results[mode + "_mixed"], results[mode + "_mixed_reversed"], "order")
    assert lib.FreeGpu() == 0


def test_stage_windows_and_batches():
    """GHOSTM_PILEUP_SCRATCH_MB=1, the smallest budget, holds 8192 positions (256
    tiles of 32; a single tile per window cannot be asked for in megabytes): the
    edge shapes moved onto the window edge at 8192 in a chunk of three windows,
    with upload batches of 7 hits, against the model and against one window."""
    lib = native.load()
    sets = rp.edge_sets(0, offset=8192 - 64, residues=17000)
    first = sets["frame_mixed"]
    rc.stage_setup(lib, first)
    gpu = rp.gpu_call(lib)
    for name in ("frame_mixed", "band_mixed", "frame_copies_300", "frame_shift_after_group", "frame_up_at_tile_start"):
        rs = sets[name]
        want = rp.model(rs)
        with _Env(rp.EDGE_ENV):
            whole = rp.pileup_via(gpu, rs)
        with _Env(dict(rp.EDGE_ENV, GHOSTM_PILEUP_SCRATCH_MB="1", GHOSTM_PILEUP_BATCH_HITS="7")):
            s0 = stage_read_pileup_stats()
            got = rp.pileup_via(gpu, rs)
            s1 = stage_read_pileup_stats()
        rp.assert_same(whole, want, ("one window", name))
        rp.assert_same(got, want, ("windows", name))
        assert s1["read_pileup_windows"] - s0["read_pileup_windows"] == 3
        if name == "frame_copies_300":   # 300 hits in batches of 7, all on tile 8198 // 32
            assert s1["read_pileup_launches"] - s0["read_pileup_launches"] == 43
        if name == "frame_up_at_tile_start":   # the pairs end window 0, the shift is charged to window 1's first position
            assert np.flatnonzero(want[3]).tolist() == [8192] and int(want[0][8188:8192].sum()) == 4
    assert lib.FreeGpu() == 0


@pytest.mark.parametrize("build", [rc.hand_band_set, lambda: rc.hand_frame_set(0)], ids=["band", "frame"])
def test_stage_refusals(build):
    """Every reason on the device entry point, the outputs untouched; no refused
    call launches anything."""
    rs = build()
    lib = native.load()
    rc.stage_setup(lib, rs)
    s0 = stage_read_pileup_stats()
    rp.check_refusals(rp.gpu_call(lib), rs, gpu=True)
    assert stage_read_pileup_stats() == s0
    assert lib.FreeGpu() == 0


@pytest.mark.parametrize("pattern", ["0xA5A5A5A5"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "readpileup_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64


def _revcomp(dna):
    return dna[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _dna_inputs():
    """Four subjects of 220-330 residues and six DNA reads of 500-800 nt: a
    stretch of a subject back-translated at a 4 % substitution rate with one
    single-nucleotide indel planted in its middle, between flanks; every other
    read reverse-complemented."""
    r = random.Random(20261103)
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
        reads.append((f"read{i}", _revcomp(dna) if i % 2 else dna))
    return subjects, reads


def _protein_inputs():
    """Five subjects of 300-340 residues; read 0 is subject 0 end to end (300
    letters) at a 4 % substitution rate, the others stretches of 280-320 letters
    of their subjects with a planted indel (band_cases.planted)."""
    r = random.Random(20261104)
    subjects = [("long0", bc.rand_seq(r, 300))] + [(f"subj{i}", bc.rand_seq(r, r.randint(300, 340))) for i in range(1, 5)]
    reads = [("whole0", bc.mutate(r, subjects[0][1], 0.04))]
    for i in range(1, 5):
        reads.append((f"read{i}", bc.planted(r, r.randint(280, 320), subjects[i][1])[0]))
    return subjects, reads


def _write_fasta(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(f">{name}\n{seq}\n")


def _open(db, reads, dna, y="0"):
    s = Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y])
    s.set_db_fasta(db)
    s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
    return s


def _check(s, frame, dna, fresh=True):
    """read_pileup(frame) of a session that has run against the Python model fed
    with the session's own paths and sources; fresh: this call makes the
    result, so the counters move by what the words say. Returns (result, model)."""
    path, ops = s.hits_frame() if frame else s.hits_band()
    before = s.read_pileup_stats()
    got = s.read_pileup(frame)
    st = s.read_pileup_stats()
    want = rp.session_model(s, W, STEP, frame, path, ops, dna=dna)
    subj, depth, ident, cons, shifts = got
    assert np.array_equal(subj, want[0]), (subj, want[0])
    rp.assert_same((depth, ident, cons, shifts), want[1:5], ("session", frame))
    hits = s.hits()
    assert len(hits) >= 4 and np.array_equal(subj["hits"], np.bincount(hits["db_id"], minlength=len(subj)))
    cols, nshift = rp.charged_columns(path, ops)
    assert int(subj["depth_sum"].sum()) == cols == int(depth.sum()) > 0
    rows = (s.hits_frame_rows() if frame else s.hits_band_rows())[0]
    assert int(subj["identities_sum"].sum()) == int(rows["identities"].sum())   # the fixtures hold codes below 25 only
    assert int(subj["shifts_sum"].sum()) == nshift == int(shifts.sum())
    if fresh:
        assert st["read_pileup_columns"] - before["read_pileup_columns"] == cols
        assert st["read_pileup_shifts"] - before["read_pileup_shifts"] == nshift
        assert st["read_pileup_launches"] > before["read_pileup_launches"] and st["seconds_read_pileup"] > 0
    else:
        assert st == before
    again = s.read_pileup(frame)   # kept: the second call launches nothing
    assert s.read_pileup_stats() == st
    for a, b in zip(again, got):
        assert np.array_equal(a, b)
    for i in np.flatnonzero(subj["hits"])[:2]:
        prof = s.read_subject_profile(frame, int(i))
        a, n = int(subj["offset"][i]), int(subj["length"][i])
        assert prof.shape == (n, 32) and np.array_equal(prof, want[5][a:a + n])
        assert np.array_equal(prof[:, :27].sum(axis=1), depth[a:a + n])
    for f in TILE_STATS:   # the tile pile-up's counters stay 0 when only the new pass runs
        assert s.stats()[f] == 0, f
    return got, want


@pytest.fixture(scope="module")
def dna_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("readpileup_dna")
    subjects, reads = _dna_inputs()
    _write_fasta(os.path.join(str(tmp), "db.fa"), subjects)
    _write_fasta(os.path.join(str(tmp), "reads.fa"), reads)
    return dict(tmp=str(tmp), db=os.path.join(str(tmp), "db.fa"), fa=os.path.join(str(tmp), "reads.fa"),
                subjects=subjects, reads=reads)


@pytest.fixture(scope="module")
def protein_files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("readpileup_prot")
    subjects, reads = _protein_inputs()
    _write_fasta(os.path.join(str(tmp), "db.fa"), subjects)
    _write_fasta(os.path.join(str(tmp), "reads.fa"), reads)
    return dict(tmp=str(tmp), db=os.path.join(str(tmp), "db.fa"), fa=os.path.join(str(tmp), "reads.fa"),
                subjects=subjects, reads=reads)


def test_session_dna_band_and_frame(dna_files):
    with _open(dna_files["db"], dna_files["reads"], True) as s:
        s.run()
        for f in STATS:   # nothing new runs until the read-level pile-up is asked for
            assert s.read_pileup_stats()[f] == 0, f
        band, _ = _check(s, False, True)
        assert int(band[4].sum()) == 0 and (band[0]["shifts_sum"] == 0).all()
        frame, _ = _check(s, True, True)
        info = s.frame_info()
        assert int(frame[0]["shifts_sum"].sum()) == int(info["shifts"].sum()) > 0   # the planted indels
        launches = s.read_pileup_stats()["read_pileup_launches"]
        # a change of the frameshift cost recomputes the frame pile-up only; with the largest cost no path shifts
        s.set_frame_shift(-(1 << 20))
        s.read_pileup(False)
        assert s.read_pileup_stats()["read_pileup_launches"] == launches
        free = s.read_pileup(True)
        assert s.read_pileup_stats()["read_pileup_launches"] > launches and int(free[4].sum()) == 0
        assert int(free[0]["shifts_sum"].sum()) == 0
        _check(s, True, True, fresh=False)
        # a change of band recomputes both
        launches = s.read_pileup_stats()["read_pileup_launches"]
        s.set_band(5)
        narrow, _ = _check(s, False, True)
        assert s.read_pileup_stats()["read_pileup_launches"] > launches
        _check(s, True, True)
        # the old pass alone leaves the new counters as they are
        st = s.read_pileup_stats()
        s.pileup()
        assert s.read_pileup_stats() == st and s.stats()["pileup_launches"] >= 1


def test_session_protein_and_the_long_read(protein_files):
    """Protein reads of about 300 letters; read 0 matches subject 0 end to end:
    its read-level pile-up covers at least 254 positions of that subject (two
    full tiles' worth), the tile pile-up at most 127."""
    with _open(protein_files["db"], protein_files["reads"], False) as s:
        s.run()
        got, want = _check(s, False, False)
        hits = s.hits()
        assert (hits["db_id"] == 0).sum() == 1   # one hit per subject of a read's name group
        assert int(want[0]["covered"][0]) >= 254   # the fixture meets the bound on the model alone
        assert int(got[0]["covered"][0]) >= 254
        with pytest.raises(GhostmError, match="tiled"):   # refused where hits_frame() is
            s.read_pileup(True)
        with pytest.raises(GhostmError, match="tiled"):
            s.read_subject_profile(True, 0)
        tile = s.pileup()
        assert 0 < int(tile[0]["covered"][0]) <= 127


# ------------------------------------------------------------ -y 16 to -y 19
def _search(files, dna, y, out, extra=()):
    cmd = [cases.GHOSTM, "search", "-q", "d" if dna else "p", "-w", str(3 * W if dna else W), "-T", str(STEP), "-y", y,
           "-D", "0", *extra, "-f", files["db"], files["fa"], out]
    return subprocess.run(cmd, capture_output=True)


def _want_text(names, pile, frame, consensus):
    subj, depth, ident, cons, shifts = pile
    lines = []
    for i in np.flatnonzero(subj["hits"]):
        x = subj[i]
        cols = [names[i].encode()] + [str(int(x[f])).encode() for f in
                                      ("length", "hits", "covered", "depth_sum", "identities_sum", "max_depth")]
        if frame:
            cols.append(str(int(x["shifts_sum"])).encode())
        if consensus:
            a, n = int(x["offset"]), int(x["length"])
            cols.append(consensus_text(cons[a:a + n], depth[a:a + n]))
        lines.append(b"\t".join(cols) + b"\n")
    return b"".join(lines)


def test_y16_to_y19_through_search(dna_files, tmp_path):
    names = [x[0] for x in dna_files["subjects"]]
    with _open(dna_files["db"], dna_files["reads"], True) as s:
        s.run()
        piles = {False: s.read_pileup(False), True: s.read_pileup(True)}
        tile = s.pileup()
    with _open(dna_files["db"], dna_files["reads"], True) as s:
        s.set_band(9)
        s.set_frame_shift(-3)
        s.run()
        tuned = s.read_pileup(True)
    assert int(piles[True][0]["shifts_sum"].sum()) > 0
    for y, frame, consensus in (("16", False, False), ("17", False, True), ("18", True, False), ("19", True, True)):
        out = str(tmp_path / f"y{y}.out")
        r = _search(dna_files, True, y, out)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out, "rb").read()
        assert text == _want_text(names, piles[frame], frame, consensus) and text.count(b"\n") >= 3, y
        with _open(dna_files["db"], dna_files["reads"], True, y=y) as s:   # the session writes the same bytes
            s.run()
            assert s.output() == text and s.read_pileup_stats()["read_pileup_launches"] >= 1
    out = str(tmp_path / "tuned.out")   # -B and -F apply
    assert _search(dna_files, True, "19", out, ("-B", "9", "-F", "3")).returncode == 0
    assert open(out, "rb").read() == _want_text(names, tuned, True, True)
    # -y 10 / -y 11 of the same inputs are the tile pile-up's, as before
    for y in ("10", "11"):
        out = str(tmp_path / f"y{y}.out")
        assert _search(dna_files, True, y, out).returncode == 0
        want = _want_text(names, tile + (None,), False, y == "11")
        assert open(out, "rb").read() == want


def test_y18_on_a_protein_set_is_y13s_error(protein_files, tmp_path):
    errs = {}
    for y in ("13", "18", "19"):
        out = str(tmp_path / f"p{y}.out")
        r = _search(protein_files, False, y, out)
        errs[y] = r.stderr
        assert b"tiled" in r.stderr and (not os.path.exists(out) or os.path.getsize(out) == 0), y
    assert errs["18"] == errs["13"] == errs["19"]
    out = str(tmp_path / "p16.out")   # the band pile-up needs no DNA
    assert _search(protein_files, False, "16", out).returncode == 0
    with _open(protein_files["db"], protein_files["reads"], False) as s:
        s.run()
        pile = s.read_pileup(False)
    assert open(out, "rb").read() == _want_text([x[0] for x in protein_files["subjects"]], pile, False, False)


# ------------------------------------------------------------ shards
def test_two_shards_add_up(data_root):
    d = tx.build_fixture(data_root, 75)

    def run(shard):
        with Session(["-i", f"{d}/q", "-d", f"{d}/db", "-o", os.devnull, "-D", "0"], shard=shard) as s:
            s.run()
            return s.read_pileup(False), len(s.hits())
    whole, n = run(None)
    parts = [run((r, 2)) for r in range(2)]
    assert all(p[1] > 0 for p in parts) and sum(p[1] for p in parts) == n
    for k in (1, 2, 4):   # depth, identities, shifts
        assert np.array_equal(sum(p[0][k].astype(np.uint64) for p in parts), whole[k]), k
    for f in ("hits", "depth_sum", "identities_sum", "shifts_sum"):
        assert np.array_equal(sum(p[0][0][f].astype(np.uint64) for p in parts), whole[0][f]), f
    assert int(whole[1].sum()) > 0
