"""The mate-pair join on the device: k_pair_join at the stage level (PairJoinGpu
against GhostmPairJoinHost, every word equal: the small shapes, the pairs at the
class borders of 64 and 1024 hits and past them, one call that mixes all
classes, the random calls, the batch cuts by both limits, the counters, the
refusals, the LDS poison build); the session post-pass (Session.pair_join,
pair_lca) on a tiny database with two pairs of reads, as protein and as DNA;
the profile counting fragments; -y 26, -y 27, -j and -J; a session with mates
off prints what it printed."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cases
import frame_cases as fc
import pair_cases as pc
import pileup_cases
from ghostm_amd import (CULL_KEPT, PAIR_HIT_DTYPE, GhostmError, pair_join, pair_join_host, read_lca_host,
                        stage_pair_join_stats)
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SHAPES = pc.shape_cases()
_Env = pileup_cases.pr_env
NONE = pc.NONE


def _counted(case, want):
    """PairJoinGpu on the case, the counters checked against the records"""
    s0 = stage_pair_join_stats()
    got = pair_join(*case)
    s1 = stage_pair_join_stats()
    pb = case[0].astype(np.int64)
    sizes = pb[2::2] - pb[:-1:2]
    cand, partner, pairs = want
    taken = 0
    for p in range(len(sizes)):
        taken += int((partner[pb[2 * p + 1]:pb[2 * p + 2]] != NONE).sum())
    assert s1["pair_hits"] - s0["pair_hits"] == int(sizes.sum())
    assert s1["pair_pairs"] - s0["pair_pairs"] == int((sizes > 0).sum())
    assert s1["pair_joined"] - s0["pair_joined"] == int(pairs["joined"].sum())
    assert s1["pair_taken"] - s0["pair_taken"] == taken
    assert (s1["pair_launches"] > s0["pair_launches"]) == bool((sizes > 0).any())
    assert s1["seconds_pair"] >= s0["seconds_pair"]
    return got, s1["pair_launches"] - s0["pair_launches"]


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_equals_host_model_on_the_shapes(name):
    case = SHAPES[name]
    want = pair_join_host(*case)
    pc.expected_shapes(name, want)
    got, launches = _counted(case, want)
    pc.assert_same(got, want, name)
    assert launches == (name != "empty_pair")


@pytest.mark.parametrize("n", pc.SIZES)
def test_stage_equals_host_model_at_the_class_borders(n):
    case = pc.sized_pair(n)
    want = pair_join_host(*case)
    assert len(case[2]) == n and want[2]["joined"][0] > n // 8
    got, launches = _counted(case, want)
    pc.assert_same(got, want, n)
    assert launches == 1


@pytest.mark.parametrize("max_span,orient", [(600, 1), (1 << 24, 0), (1, 1)])
def test_stage_mixed_and_random_pairs(max_span, orient):
    """one call that mixes all classes, and the host test's random calls joined into one call"""
    for what, case in (("mixed", pc.mixed_call(max_span, orient)),
                       ("random", pc.join(pc.random_calls(150), max_span, orient))):
        want = pair_join_host(*case)
        got, launches = _counted(case, want)
        pc.assert_same(got, want, (what, max_span, orient))
        assert launches == 1


def test_stage_batch_cuts():
    """The mixed call in batches of three pairs, and twelve pairs of the
    device-memory class in batches cut by a budget of one megabyte: the result
    does not depend on the cuts."""
    case = pc.mixed_call()
    want = pair_join_host(*case)
    pb = case[0].astype(np.int64)
    sizes = pb[2::2] - pb[:-1:2]
    with _Env({"GHOSTM_PAIR_BATCH_PAIRS": "3"}):
        got, launches = _counted(case, want)
    pc.assert_same(got, want, "batches of three pairs")
    assert launches == sum(1 for b in range(0, len(sizes), 3) if sizes[b:b + 3].sum() > 0) > 3
    big = pc.join([pc.sized_pair(3000, seed=s) for s in range(12)], 600, 1)
    big_want = pair_join_host(*big)
    # a pair's bytes: 32 a hit going up, 20 a hit coming back, 32 for its record, borders and list entry
    cost = np.full(12, 3000 * 52 + 32)
    cuts, used = 1, 0
    for c in cost:
        if used and used + c > 1 << 20:
            cuts, used = cuts + 1, 0
        used += c
    with _Env({"GHOSTM_PAIR_SCRATCH_MB": "1"}):
        got, launches = _counted(big, big_want)
    pc.assert_same(got, big_want, "batches of a megabyte")
    assert launches == cuts == 2
    got, launches = _counted(big, big_want)
    pc.assert_same(got, big_want, "the twelve in one batch")
    assert launches == 1


def test_stage_hits_outside_every_pair_and_refusals():
    """Hits before the first pair and after the last keep the outputs' bytes;
    every reason on the device entry point, the outputs untouched; no refused
    call launches anything or counts."""
    pb, off, h, max_span, orient = SHAPES["joined"]
    outer = np.concatenate([h[:1], h, h[1:]])
    got = pair_join(pb + 1, off, outer, max_span, orient, out=pc.filled_outputs(len(outer), 1))
    want = pair_join_host(pb + 1, off, outer, max_span, orient, out=pc.filled_outputs(len(outer), 1))
    pc.assert_same(got, want, "outer hits")
    assert got[1].tolist() == [pc.FILL, 2, 1, pc.FILL]
    s0 = stage_pair_join_stats()
    pc.check_refusals("PairJoinGpu")
    with pytest.raises(GhostmError, match="PairJoinGpu: .*param: orient"):
        pair_join(*SHAPES["joined"][:4], orient=2)
    assert stage_pair_join_stats() == s0


@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "pair_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
A, B = 0, 1   # the subjects' db_ids
NODES = [(1, 1), (10, 1), (100, 10), (110, 10)]   # (taxid, parent taxid): two species of one genus
TAXID = np.array([t for t, _ in NODES], dtype=np.uint32)
PARENT = np.array([[t for t, _ in NODES].index(p) for _, p in NODES], dtype=np.uint32)
GENUS, SP_A, SP_B = 1, 2, 3   # node indices
SUBJECT_NODE = np.array([SP_A, SP_B], dtype=np.uint32)


def _revcomp(dna):
    return dna[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _inputs():
    """Subject A: 300 random residues. Subject B: 150 of its own, then a copy of
    A's first 100. Pair 0: mate 1 is A's first 100 residues (it hits A and B
    alike), mate 2 A's residues 150 to 249. Pair 1: mate 1 is noise, mate 2 B's
    own first 100. The same as DNA, back-translated, mate 2 reverse-complemented."""
    r = random.Random(20270107)
    sub_a = fc.rand_prot(r, 300)
    own_b = fc.rand_prot(r, 150)
    subjects = [("subA", sub_a), ("subB", own_b + sub_a[:100])]
    prot = [("p0/1", sub_a[:100]), ("p0/2", sub_a[150:250]), ("p1/1", fc.rand_prot(r, 100)), ("p1/2", own_b[:100])]
    dna = [(n, _revcomp(fc.back_translate(s)) if n.endswith("/2") else fc.back_translate(s)) for n, s in prot]
    same = [(n, fc.back_translate(s)) for n, s in prot]   # mate 2 left on mate 1's strand
    return subjects, prot, dna, same


def _write(path, records):
    with open(path, "w") as f:
        for name, seq in records:
            f.write(f">{name}\n{seq}\n")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("pairjoin"))
    subjects, prot, dna, same = _inputs()
    out = dict(tmp=tmp, db=os.path.join(tmp, "db.fa"), prot=prot, dna=dna, same=same,
               nodes=os.path.join(tmp, "nodes.tsv"), map=os.path.join(tmp, "map.tsv"))
    _write(out["db"], subjects)
    for key in ("prot", "dna", "same"):
        recs = out[key]
        out[key + "_fa"] = os.path.join(tmp, key + ".fa")
        out[key + "_r1"] = os.path.join(tmp, key + "_r1.fa")
        out[key + "_r2"] = os.path.join(tmp, key + "_r2.fa")
        _write(out[key + "_fa"], recs)
        _write(out[key + "_r1"], recs[0::2])
        _write(out[key + "_r2"], recs[1::2])
    with open(out["nodes"], "w") as f:
        for t, p in NODES:
            f.write(f"{t}\t{p}\n")
    with open(out["map"], "w") as f:
        f.write("subA\t100\nsubB\t110\n")
    return out


def _open(files, dna, y="0", mates=(True, 1000), reads=None, tax=True):
    s = Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y, "-b", "3"])
    s.set_db_fasta(files["db"])
    if tax:
        s.set_taxonomy(TAXID, PARENT, SUBJECT_NODE)
    s.set_cull(2, 100)   # mate 1's two hits lie on one stretch: both are kept
    if mates is not None:
        s.set_mates(*mates)
    reads = files["dna" if dna else "prot"] if reads is None else reads
    s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
    return s


def _session_model(s, reads, frame, dna, max_insert=1000):
    """GhostmPairJoinHost on the records the contract names, made here from the
    session's hits, paths, tile table and cull. Returns (the call's arguments, its result)."""
    hits, tiles = s.hits(), s.query_tiles()
    t = tiles[s.hits_band_rows()[0]["query_record"]]
    path = s.hits_frame()[0] if frame else s.hits_band()[0]
    cull = s.read_cull(frame)
    info = s.frame_info() if dna else None
    n = len(hits)
    rec = np.zeros(n, dtype=PAIR_HIT_DTYPE)
    rec["node"] = NONE
    for h in range(n):
        if cull["status"][h] != CULL_KEPT:
            continue
        q0, q1 = int(path["q_start"][h]), int(path["q_end"][h])
        if dna:
            g, strand, nt = int(t["frame"][h]) % 3, int(info["strand"][h]), int(info["read_nt"][h])
            p0, p1 = (q0, q1) if frame else (3 * q0 + g, 3 * q1 + g + 2)
            q0, q1 = sorted((nt - 1 - p0, nt - 1 - p1) if strand else (p0, p1))
        rec[h] = (hits["db_id"][h], SUBJECT_NODE[hits["db_id"][h]], path["score"][h], q0, q1, path["s_start"][h],
                  path["s_end"][h], int(t["frame"][h]) // 3 if dna else 0)
    record = t["record"].astype(np.int64)
    assert (np.diff(record) >= 0).all()
    begin, offset, first = [], [], []
    for p in sorted(set((record >> 1).tolist())):
        begin += [int(np.searchsorted(record, 2 * p)), int(np.searchsorted(record, 2 * p + 1))]
        offset.append(len(reads[2 * p][1]))
        first.append(2 * p)
    begin.append(n)
    args = (np.array(begin, dtype=np.uint32), np.array(offset, dtype=np.uint32), rec,
            max(1, max_insert // 3) if dna else max_insert, 1 if dna else 0)
    return args, pair_join_host(*args), np.array(first, dtype=np.uint32)


def _want_text(names, lca, pairs):
    taxid = lambda n: 0 if n == NONE else int(TAXID[n])   # noqa: E731
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
        name.encode(), taxid(o["node"]), o["depth"], o["votes"], o["support"], taxid(o["lca"]), o["candidates"],
        o["unmapped"], o["best_score"], j["mates"], j["joined"], j["best_span"]) for name, o, j in zip(names, lca, pairs))


def _two_pairs(files, dna, tmp_path):
    frame, y_pair, key = (True, "27", "dna") if dna else (False, "26", "prot")
    reads = files[key]
    with _open(files, dna, y="13" if dna else "12") as s:
        s.run()
        assert s.pair_join_stats()["pair_launches"] == 0   # the path styles ask for no join
        hits = s.hits()
        alone, alone_begin = s.read_lca(frame, with_begin=True)
        names = [s.query_tiles()[s.hits_band_rows()[0]["query_record"]]["record"][b] for b in alone_begin[:-1]]
        assert names == [0, 1, 3] and alone["node"].tolist() == [GENUS, SP_A, SP_B]   # three reads; mate 1 alone: the genus
        kept = int((s.read_cull(frame)["status"] == CULL_KEPT).sum())
        cand, partner, pairs, begin, record = s.pair_join(frame)
        args, want, first = _session_model(s, reads, frame, dna)
        pc.assert_same((cand, partner, pairs), want, "session")
        assert begin.tolist() == args[0].tolist() and record.tolist() == first.tolist() == [0, 2]
        # pair 0: mate 1's hit of A joins mate 2's, its hit of B stays alone; pair 1: mate 2 only
        assert pairs["joined"].tolist() == [1, 0] and pairs["mates"].tolist() == [3, 2] and 240 <= pairs["best_span"][0] <= 250
        m1 = [h for h in range(begin[0], begin[1]) if cand["score"][h]]
        assert sorted(hits["db_id"][m1].tolist()) == [A, B] and begin[3] == begin[2]   # pair 1 has no hit of mate 1
        joined = [h for h in m1 if partner[h] != NONE]
        assert hits["db_id"][joined].tolist() == [A] and begin[1] <= partner[joined[0]] < begin[2]
        assert partner[partner[joined[0]]] == joined[0] and cand["score"][partner[joined[0]]] == 0
        st = s.pair_join_stats()
        assert (st["pair_launches"], st["pair_pairs"], st["pair_hits"], st["pair_joined"], st["pair_taken"]) == (
            1, 2, len(hits), 1, 1)
        lca = s.pair_lca(frame)
        assert np.array_equal(lca, read_lca_host(PARENT, begin[::2], cand, 10, 100))
        assert lca["node"].tolist() == [SP_A, SP_B] and lca["votes"].tolist() == [1, 1] and lca["candidates"][0] == 2
        # the profile counts fragments
        rec, final, summary = s.taxon_profile(frame)
        assert summary["reads"] == 2 and final.tolist() == [SP_A, SP_B]
        launches = s.read_lca_stats()["lca_launches"]
        s.pair_join(frame), s.pair_lca(frame), s.set_mates(True, 1000)   # kept; no change
        assert s.pair_join_stats() == st and s.read_lca_stats()["lca_launches"] == launches
        s.set_mates(True, 600 if dna else 200)   # under the fragment's 250 residues: no join, the genus again
        cand2, partner2, pairs2, _, _ = s.pair_join(frame)
        pc.assert_same((cand2, partner2, pairs2), _session_model(s, reads, frame, dna, 600 if dna else 200)[1], "short insert")
        assert pairs2["joined"].tolist() == [0, 0] and s.pair_lca(frame)["node"].tolist() == [GENUS, SP_B]
        assert s.pair_join_stats()["pair_launches"] == 2 and s.read_cull_stats()["cull_launches"] == 1   # the cull stays
        s.set_mates(False, 1000)   # off: reads again, and the pair passes say why they do not run
        assert s.taxon_profile(frame)[2]["reads"] == 3
        with pytest.raises(GhostmError, match="mates: they are off"):
            s.pair_join(frame)
        with pytest.raises(GhostmError, match="mates"):
            s.pair_lca(frame)
        with pytest.raises(GhostmError, match="param"):
            s.set_mates(True, 0)
        s.set_mates(True, 1000)
        s.set_cull(1, 50)   # a change of the cull drops the join: mate 1's second hit is culled
        s.pair_join(frame)
        assert int((s.read_cull(frame)["status"] == CULL_KEPT).sum()) == kept - 1 and s.pair_join_stats()["pair_launches"] == 3
        s.set_cull(2, 100)
        text = _want_text(["p0/1", "p1/1"], s.pair_lca(frame), s.pair_join(frame)[2])
    assert text.startswith(b"p0/1\t100\t2\t1\t1\t100\t2\t0\t") and b"\np1/1\t110\t2\t1\t1\t110\t1\t0\t" in text
    with _open(files, dna, y=y_pair) as s:
        s.run()
        assert s.output() == text and s.pair_join_stats()["pair_launches"] == 1
    # the command form: -j on the interleaved file, -J on the two files, byte for byte
    base = [cases.GHOSTM, "search", "-q", "d" if dna else "p", "-w", str(3 * W if dna else W), "-T", str(STEP), "-b", "3",
            "-D", "0", "-K", "2", "-C", "100", "-n", files["nodes"], "-a", files["map"], "-f", files["db"]]
    outs = {}
    for what, extra in (("j", ["-y", y_pair, "-j", files[key + "_fa"]]),
                        ("J", ["-y", y_pair, "-J", "-I", "1000", files[key + "_r1"], files[key + "_r2"]]),
                        ("j24", ["-y", "25" if dna else "24", "-j", files[key + "_fa"]]),
                        ("reads24", ["-y", "25" if dna else "24", files[key + "_fa"]])):
        out_path = str(tmp_path / (what + ".out"))
        r = subprocess.run(base + extra + [out_path], capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[what] = open(out_path, "rb").read()
    assert outs["j"] == text and outs["J"] == text
    assert outs["j24"] != outs["reads24"] and outs["j24"] and outs["reads24"]   # fragments, not reads


def test_session_protein_two_pairs(files, tmp_path):
    _two_pairs(files, False, tmp_path)


def test_session_dna_two_pairs(files, tmp_path):
    _two_pairs(files, True, tmp_path)
    # mate 2 left on mate 1's strand: the same hits, no join
    with _open(files, True, reads=files["same"]) as s:
        s.run()
        cand, partner, pairs, begin, _ = s.pair_join(True)
        assert pairs["joined"].tolist() == [0, 0] and pairs["mates"].tolist() == [3, 2] and (partner == NONE).all()
        assert s.pair_lca(True)["node"].tolist() == [GENUS, SP_B]


def test_session_refusals_and_two_files(files):
    with _open(files, False, mates=(True, 1000)) as s:
        s.set_queries_fasta_mates(files["prot_r1"], files["prot_r2"], width=W, tile_step=STEP)
        s.run()
        two = s.pair_join(False)
        s.set_queries_fasta(files["prot_fa"], width=W, tile_step=STEP)
        s.run()
        for got, want in zip(s.pair_join(False), two):
            assert np.array_equal(got, want)
        # files of different record counts are refused and the set stays
        with pytest.raises(GhostmError, match=r"mates: .* has 4 records, .* has 2"):
            s.set_queries_fasta_mates(files["prot_fa"], files["prot_r2"], width=W, tile_step=STEP)
        assert len(s.query_tiles()) == 4
        # an odd number of source records, an untiled set
        s.set_queries([x[1] for x in files["prot"][:3]], [x[0] for x in files["prot"][:3]], width=W, tile_step=STEP)
        s.run()
        with pytest.raises(GhostmError, match="mates: 3 source records"):
            s.pair_join(False)
        with pytest.raises(GhostmError, match="mates: 3 source records"):
            s.taxon_profile(False)
        s.set_queries([x[1] for x in files["prot"]], [x[0] for x in files["prot"]], width=W)
        s.run()
        with pytest.raises(GhostmError, match="mates: the query set is not tiled"):
            s.pair_join(False)
    with _open(files, False, tax=False) as s:   # without a taxonomy the join runs, the assignment does not
        s.run()
        assert s.pair_join(False)[2]["joined"].tolist() == [1, 0] and (s.pair_join(False)[0]["node"] == NONE).sum() >= 3
        with pytest.raises(GhostmError, match="taxonomy"):
            s.pair_lca(False)


def test_usage_errors():
    """-j, -J and -I without -T, -j with -J, -I without mates, -y 26 without
    mates or without a taxonomy: 1 and the usage text, before any device call;
    aln names search."""
    base = [cases.GHOSTM, "search", "-f", "db.fa"]
    tax = ["-n", "nodes", "-a", "map"]
    for extra in (["-j"], ["-J"], ["-T", "64", "-j", "-J"], ["-T", "64", "-I", "500"], ["-j", "-I", "500"],
                  ["-T", "64", "-j", "-I", "0"], ["-T", "64", "-y", "26"] + tax, ["-T", "64", "-j", "-y", "27"],
                  ["-T", "64", "-J"] + tax):
        r = subprocess.run(base + extra + ["q.fa", "o"], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"ghostm (") and b"\nsearch: " in r.stderr, (extra, r)
    for y in ("26", "27"):
        r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", "o", "-y", y], capture_output=True)
        assert r.returncode == 0 and b"search" in r.stderr and b"mates" in r.stderr, r


def _outcome(files, dna, y, mates):
    """what a session of style y gives: ("ok", text, hits, the untimed stats, pair launches), or ("refused", message)"""
    try:
        with _open(files, dna, y=y, mates=mates) as s:
            s.run()
            stats = {k: v for k, v in s.stats().items() if not k.startswith("seconds")}
            return "ok", s.output(), s.hits().tobytes(), stats, s.pair_join_stats()["pair_launches"]
    except GhostmError as e:
        return "refused", str(e)


@pytest.mark.parametrize("dna", [False, True], ids=["protein", "dna"])
def test_mates_off_changes_nothing(files, dna):
    """With mates off (never mentioned, or an insert limit given with them off)
    the taxon lines and the profile, and the styles under them, print the same
    text from the same hits and counters; no join is launched."""
    for y in ("0", "12", "20", "22", "24") + (("13", "23", "25") if dna else ()):
        plain = _outcome(files, dna, y, None)
        got = _outcome(files, dna, y, (False, 300))
        assert plain[0] == "ok" and got == plain and plain[4] == 0, y
    with _open(files, dna, y="24", mates=None) as s:
        s.run()
        reads = s.output()
    with _open(files, dna, y="24", mates=(True, 1000)) as s:
        s.run()
        assert s.output() != reads and s.pair_join_stats()["pair_launches"] == 1
