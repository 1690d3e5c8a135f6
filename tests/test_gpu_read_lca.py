"""The per-read taxonomic assignment on the device: k_read_lca_wave and k_read_lca
at the stage level (ReadLcaGpu against GhostmReadLcaHost, every record equal:
the small shapes, every tree, the reads at the class borders of 64 and 1024
candidates and past them, one call that mixes all classes, the batch cuts, a
second taxonomy, the refusals, FreeGpu, the LDS poison build); the session
post-pass (Session.read_lca) on a read that carries two genes, as protein and
as DNA with a planted indel, with tile groups; -y 22 and -y 23; the file form;
a session without a taxonomy prints what it printed."""
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
import readlca_cases as lc
from ghostm_amd import (CULL_KEPT, LCA_HIT_DTYPE, LCA_OUT_DTYPE, GhostmError, native, read_lca, read_lca_host,
                        set_taxonomy_gpu, stage_read_lca_stats)
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")
SHAPES = lc.shape_cases()
TREE_CASES = lc.tree_cases()
_Env = pc.pr_env
NONE = lc.NONE


def _counted(case, want):
    """ReadLcaGpu on the case (its taxonomy made resident), the counters checked against the records"""
    set_taxonomy_gpu(case[0])
    s0 = stage_read_lca_stats()
    got = read_lca(*case[1:])
    s1 = stage_read_lca_stats()
    rb = case[1].astype(np.int64)
    assert s1["lca_hits"] - s0["lca_hits"] == int(rb[-1] - rb[0])
    assert s1["lca_reads"] - s0["lca_reads"] == int((np.diff(rb) > 0).sum())
    assert s1["lca_votes"] - s0["lca_votes"] == int(want["votes"].sum())
    assert s1["lca_assigned"] - s0["lca_assigned"] == int((want["node"] != NONE).sum())
    assert (s1["lca_launches"] > s0["lca_launches"]) == bool((want["candidates"] > 0).any())
    return got, s1["lca_launches"] - s0["lca_launches"]


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("name", list(SHAPES))
def test_stage_equals_host_model_on_the_shapes(name):
    case = SHAPES[name]
    want = read_lca_host(*case)
    lc.expected_shapes(name, want)
    got, _ = _counted(case, want)
    lc.assert_same(got, want, name)


@pytest.mark.parametrize("name", list(TREE_CASES))
def test_stage_equals_host_model_on_the_trees(name):
    case = TREE_CASES[name]
    want = read_lca_host(*case)
    got, _ = _counted(case, want)
    lc.assert_same(got, want, name)


@pytest.mark.parametrize("n", lc.SIZES)
def test_stage_equals_host_model_at_the_class_borders(n):
    case = lc.sized_read(n)
    want = read_lca_host(*case)
    assert want["candidates"][0] == n
    got, launches = _counted(case, want)
    lc.assert_same(got, want, n)
    assert launches == 1


@pytest.mark.parametrize("top_pct,support_pct", [(10, 100), (0, 51), (100, 60)])
def test_stage_mixed_and_random_reads(top_pct, support_pct):
    """one call that mixes all classes, and the host test's random reads joined into one call"""
    for what, case in (("mixed", lc.mixed_call(top_pct, support_pct)),
                       ("random", lc.join(lc.random_calls(150), top_pct, support_pct))):
        want = read_lca_host(*case)
        got, launches = _counted(case, want)
        lc.assert_same(got, want, (what, top_pct, support_pct))
        assert launches == 1


def test_stage_batch_cuts_and_a_second_taxonomy():
    """The mixed call in batches of three reads, and twelve reads above the LDS
    class in batches cut by a budget of one megabyte: the records do not depend
    on the cuts. Then another tree: the next call uses it."""
    case = lc.mixed_call()
    want = read_lca_host(*case)
    nreads = len(case[1]) - 1
    with _Env({"GHOSTM_LCA_BATCH_READS": "3"}):
        got, launches = _counted(case, want)
    lc.assert_same(got, want, "batches of three reads")
    cand = want["candidates"].astype(np.int64)
    assert launches == sum(1 for b in range(0, nreads, 3) if cand[b:b + 3].sum() > 0) > 3
    big = lc.join([lc.sized_read(1025, seed=s) for s in range(12)], 10, 60)
    big_want = read_lca_host(*big)
    # a read's bytes: 16 a hit, a table of 10 * 2048 words above 1024 candidates, 48 for its record and list entries
    cost = np.diff(big[1].astype(np.int64)) * 16 + 10 * 2048 * 4 + 48
    cuts, used = 1, 0
    for c in cost:
        if used and used + c > 1 << 20:
            cuts, used = cuts + 1, 0
        used += c
    with _Env({"GHOSTM_LCA_SCRATCH_MB": "1"}):
        got, launches = _counted(big, big_want)
    lc.assert_same(got, big_want, "batches of a megabyte")
    assert launches == cuts == 2
    got, launches = _counted(big, big_want)
    lc.assert_same(got, big_want, "the twelve in one batch")
    assert launches == 1
    # the same hits on another tree (the binary tree has fewer nodes: fold the nodes into it)
    other = lc.TREES["binary"]
    hits = big[2].copy()
    mapped = hits["node"] != NONE
    hits["node"][mapped] %= len(other)
    second = (other, big[1], hits, 10, 60)
    second_want = read_lca_host(*second)
    assert not np.array_equal(second_want, big_want)
    got, _ = _counted(second, second_want)
    lc.assert_same(got, second_want, "the second taxonomy")
    # a refused taxonomy keeps the resident one
    with pytest.raises(GhostmError, match="SetTaxonomyGpu: taxonomy: node 1: a second root"):
        set_taxonomy_gpu(lc.BAD_TREES["two_roots"][0])
    lc.assert_same(read_lca(*second[1:]), second_want, "after a refused taxonomy")


def test_stage_refusals_and_free():
    """Every reason on the device entry point, the outputs untouched; no refused
    call launches anything or counts; FreeGpu drops the taxonomy."""
    set_taxonomy_gpu(lc.SMALL)
    read_lca(*SHAPES["one_hit"][1:])
    s0 = stage_read_lca_stats()
    lc.check_refusals("ReadLcaGpu", False)
    with pytest.raises(GhostmError, match="param"):
        read_lca(*SHAPES["one_hit"][1:3], top_pct=101)
    assert stage_read_lca_stats() == s0
    assert native.load().FreeGpu() == 0
    out = np.full(8, 0xC3C3C3C3, dtype=np.uint32).view(LCA_OUT_DTYPE)
    with pytest.raises(GhostmError, match="ReadLcaGpu: .*taxonomy: "):
        read_lca(*SHAPES["one_hit"][1:], out=out)
    assert (out.view(np.uint32) == 0xC3C3C3C3).all() and stage_read_lca_stats() == s0
    set_taxonomy_gpu(lc.SMALL)
    lc.assert_same(read_lca(*SHAPES["one_hit"][1:]), read_lca_host(*SHAPES["one_hit"]), "set again")


@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "readlca_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = 127, 64
A, A2, B, C = 0, 1, 2, 3   # the subjects' db_ids
# the taxonomy: (taxid, parent taxid) in file order; the two genes' subjects in two genera of one family
NODES = [(1, 1), (10, 1), (11, 1), (20, 10), (21, 10), (22, 11), (100, 20), (101, 20), (110, 21), (120, 22)]
SUBJECT_TAXID = {"geneA": 100, "geneA2": 101, "geneB": 110, "geneC": 120}
TAXID = np.array([t for t, _ in NODES], dtype=np.uint32)
PARENT = np.array([[t for t, _ in NODES].index(p) for _, p in NODES], dtype=np.uint32)
FAMILY = 1   # node index of taxid 10


def _inputs():
    """Four subjects of 150 residues (geneA2 a close homologue of geneA) and one
    read of about 400 letters, test_gpu_read_cull.py's: gene A at a 3 %
    substitution rate, a linker of 30 letters, gene B diverged at 12 %, 70
    letters of noise. The same read as DNA: back-translated, with one
    nucleotide planted in the middle of gene A."""
    r = random.Random(20261207)
    gene_a = fc.rand_prot(r, 150)
    subjects = [("geneA", gene_a), ("geneA2 a close homologue", fc.mutate(r, gene_a, 0.04)),
                ("geneB", fc.rand_prot(r, 150)), ("geneC", fc.rand_prot(r, 150))]
    prot = fc.mutate(r, gene_a, 0.03) + fc.rand_prot(r, 30) + fc.mutate(r, subjects[B][1], 0.12) + fc.rand_prot(r, 70)
    dna = fc.back_translate(prot)
    dna = dna[:3 * 75 + 1] + "G" + dna[3 * 75 + 1:]
    return subjects, [("read0", prot)], [("read0", dna)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("readlca"))
    subjects, prot, dna = _inputs()
    out = dict(tmp=tmp, db=os.path.join(tmp, "db.fa"), prot=prot, dna=dna, prot_fa=os.path.join(tmp, "prot.fa"),
               dna_fa=os.path.join(tmp, "dna.fa"), nodes=os.path.join(tmp, "nodes.dmp"), map=os.path.join(tmp, "map.tsv"))
    for path, records in ((out["db"], subjects), (out["prot_fa"], prot), (out["dna_fa"], dna)):
        with open(path, "w") as f:
            for name, seq in records:
                f.write(f">{name}\n{seq}\n")
    with open(out["nodes"], "w") as f:   # nodes.dmp's separators
        for t, p in NODES:
            f.write(f"{t}\t|\t{p}\t|\tno rank\t|\n")
    with open(out["map"], "w") as f:   # a later line wins; a name the database lacks is counted
        f.write("geneB\t120\nnot_here\t100\n\ngeneA 100\ngeneA2\t101\ngeneB\t110\ngeneC  120\n")
    out["subject_node"] = np.array([list(TAXID).index(SUBJECT_TAXID[n.split()[0]]) for n, _ in subjects], dtype=np.uint32)
    return out


def _open(files, dna, y="0", tax="arrays", lca=None, cull=None):
    s = Session.for_queries(["-o", os.devnull, "-D", "0", "-y", y, "-b", "3"])
    s.set_db_fasta(files["db"])
    s.set_tile_groups(True)
    if tax == "arrays":
        s.set_taxonomy(TAXID, PARENT, files["subject_node"])
    elif tax == "files":
        s.set_taxonomy_files(files["nodes"], files["map"])
    if lca is not None:
        s.set_lca(*lca)
    if cull is not None:
        s.set_cull(*cull)
    reads = files["dna" if dna else "prot"]
    s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W if dna else W, dna=dna, tile_step=STEP)
    return s


def _session_model(s, files, frame, dna, top_pct=10, support_pct=100):
    """GhostmReadLcaHost on the records the contract names, made here from the
    session's hits, paths, tile table and cull. Returns (records, read_begin)."""
    hits, tiles = s.hits(), s.query_tiles()
    band = s.hits_band()[0]
    t = tiles[s.hits_band_rows()[0]["query_record"]]
    path = s.hits_frame()[0] if frame else band
    cull = s.read_cull(frame)
    n = len(hits)
    begin = [0] + [h for h in range(1, n) if t["record"][h] != t["record"][h - 1]] + [n]
    rec = np.zeros(n, dtype=LCA_HIT_DTYPE)
    info = s.frame_info() if dna else None
    for h in range(n):
        q0 = q1 = 0
        if path["score"][h]:
            q0, q1 = int(path["q_start"][h]), int(path["q_end"][h])
            if dna:
                g, strand, nt = int(t["frame"][h]) % 3, int(info["strand"][h]), int(info["read_nt"][h])
                p0, p1 = (q0, q1) if frame else (3 * q0 + g, 3 * q1 + g + 2)
                q0, q1 = sorted((nt - 1 - p0, nt - 1 - p1) if strand else (p0, p1))
        kept = cull["status"][h] == CULL_KEPT
        rec[h] = (files["subject_node"][hits["db_id"][h]], path["score"][h] if kept else 0, q0, q1)
    begin = np.array(begin, dtype=np.uint32)
    return read_lca_host(PARENT, begin, rec, top_pct, support_pct), begin


def _want_text(names, out):
    taxid = lambda n: 0 if n == NONE else int(TAXID[n])   # noqa: E731
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
        name.encode(), taxid(o["node"]), o["depth"], o["votes"], o["support"], taxid(o["lca"]), o["candidates"],
        o["unmapped"], o["best_score"]) for name, o in zip(names, out))


def _two_genes(files, dna, tmp_path):
    frame, y_paths, y_lca = (True, "13", "23") if dna else (False, "12", "22")
    with _open(files, dna, y=y_paths) as s:
        s.run()
        assert s.read_lca_stats()["lca_launches"] == 0   # the path styles ask for no assignment
        assert s.taxonomy_info() == dict(nodes=10, subjects_mapped=4, subjects_unmapped=0, map_unmatched=0)
        out, begin = s.read_lca(frame, with_begin=True)
        want, want_begin = _session_model(s, files, frame, dna)
        lc.assert_same(out, want, "10 / 100")
        assert begin.tolist() == want_begin.tolist() and len(out) == 1
        st = s.read_lca_stats()
        assert st["lca_launches"] == 1 and st["lca_reads"] == 1 and st["lca_hits"] == len(s.hits())
        # both genes vote: the read is the family's
        kept = set(s.hits()["db_id"][s.read_cull(frame)["status"] == CULL_KEPT].tolist())
        assert {A, B} <= kept and C not in kept
        assert out["node"][0] == FAMILY and out["lca"][0] == FAMILY and out["votes"][0] >= 2 and out["depth"][0] == 1
        s.read_lca(frame)
        s.set_lca(10, 100)   # no change
        s.read_lca(frame)
        assert s.read_lca_stats() == st   # kept: nothing launched
        s.set_lca(100, 60)   # a change drops the result
        lc.assert_same(s.read_lca(frame), _session_model(s, files, frame, dna, 100, 60)[0], "100 / 60")
        assert s.read_lca_stats()["lca_launches"] == 2
        s.set_cull(2, 100)   # so does a change of the cull
        lc.assert_same(s.read_lca(frame), _session_model(s, files, frame, dna, 100, 60)[0], "cull 2 / 100")
        assert s.read_lca_stats()["lca_launches"] == 3
        with pytest.raises(GhostmError, match="param"):
            s.set_lca(10, 50)
        if not dna:
            with pytest.raises(GhostmError, match="tiled"):   # refused where hits_frame() is
                s.read_lca(True)
        # a refused taxonomy leaves the session's
        with pytest.raises(GhostmError, match="subjects"):
            s.set_taxonomy(TAXID, PARENT, files["subject_node"][:3])
        with pytest.raises(GhostmError, match="taxonomy"):
            s.set_taxonomy(np.array([1, 1], dtype=np.uint32), np.array([0, 0], dtype=np.uint32),
                           np.zeros(4, dtype=np.uint32))
        assert s.taxonomy_info()["nodes"] == 10 and s.read_lca_stats()["lca_launches"] == 3
        s.set_lca(10, 100)
        s.set_cull(1, 50)
        text = _want_text(["read0"], s.read_lca(frame))
    with _open(files, dna, y=y_lca) as s:
        s.run()
        assert s.output() == text and text.startswith(b"read0\t10\t1\t")
        assert s.read_lca_stats()["lca_launches"] == 1
    with _open(files, dna, y=y_lca, tax="files") as s:   # the file form: the same taxonomy
        assert s.taxonomy_info() == dict(nodes=10, subjects_mapped=4, subjects_unmapped=0, map_unmatched=1)
        s.run()
        assert s.output() == text
        lc.assert_same(s.read_lca(frame), out, "files")
        s.set_db_fasta(files["db"])   # a new database drops the taxonomy
        assert s.taxonomy_info()["nodes"] == 0
        with pytest.raises(GhostmError, match="taxonomy"):   # the style has nothing to print from
            s.run()
        with pytest.raises(GhostmError, match="taxonomy"):
            s.read_lca(frame)
    out_path = str(tmp_path / "lca.out")   # the command form, -p and -P at their defaults
    cmd = [cases.GHOSTM, "search", "-q", "d" if dna else "p", "-w", str(3 * W if dna else W), "-T", str(STEP), "-y", y_lca,
           "-b", "3", "-D", "0", "-g", "-n", files["nodes"], "-a", files["map"], "-p", "10", "-P", "100", "-f", files["db"],
           files["dna_fa" if dna else "prot_fa"], out_path]
    r = subprocess.run(cmd, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out_path, "rb").read() == text


def test_session_protein_two_genes(files, tmp_path):
    _two_genes(files, False, tmp_path)
    # -y 23 on a protein set: the error -y 13 gives, nothing printed
    with _open(files, False, y="23") as s:
        with pytest.raises(GhostmError, match="tiled"):
            s.run()


def test_session_dna_two_genes(files, tmp_path):
    _two_genes(files, True, tmp_path)


def test_file_refusals(files, tmp_path):
    def write(name, text):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(text)
        return path

    with _open(files, False, tax=None) as s:
        for nodes, mp, why in ((write("n1", "1 1\n2 1\n2 1\n"), files["map"], "taxonomy: nodes line 3"),
                               (write("n2", "1 1\n\n3 2\n"), files["map"], "taxonomy: nodes line 3"),
                               (files["nodes"], write("m1", "geneA 100\ngeneB 999\n"), "map: line 2"),
                               (files["nodes"], str(tmp_path / "missing"), "cannot open")):
            with pytest.raises(GhostmError, match=why):
                s.set_taxonomy_files(nodes, mp)
            assert s.taxonomy_info()["nodes"] == 0
        s.set_taxonomy_files(files["nodes"], write("m2", "geneA2 101\nother 1\nother2 1\n"))   # the name cut at the blank
        assert s.taxonomy_info() == dict(nodes=10, subjects_mapped=1, subjects_unmapped=3, map_unmatched=2)


def _outcome(files, dna, y, lca):
    """what a session of style y gives: ("ok", text, hits, the untimed stats, lca_launches), or ("refused", message)"""
    try:
        with _open(files, dna, y=y, tax=None, lca=lca) as s:
            s.run()
            stats = {k: v for k, v in s.stats().items() if not k.startswith("seconds")}
            return "ok", s.output(), s.hits().tobytes(), stats, s.read_lca_stats()["lca_launches"]
    except GhostmError as e:
        return "refused", str(e)


@pytest.mark.parametrize("dna", [False, True], ids=["protein", "dna"])
def test_no_taxonomy_changes_nothing(files, dna):
    """With no taxonomy call made (other parameters of the assignment set, but
    nothing asked of it) every existing style, -y 0 to -y 21, on the protein
    set and on the DNA set (the frame styles 13, 15, 18, 19 and 21 run there and
    are refused on the protein set), gives what a session that never heard of
    the feature gives: the same text, hits and counters, or the same refusal;
    nothing is launched."""
    ran = []
    for y in range(22):
        plain = _outcome(files, dna, str(y), None)
        got = _outcome(files, dna, str(y), (30, 60))
        assert got == plain, y
        if plain[0] == "ok":
            assert plain[4] == 0
            ran.append(y)
    frame_styles = {13, 15, 18, 19, 21}
    assert {0, 6, 7, 8, 9, 10, 11, 12, 14, 16, 17, 20} <= set(ran)
    assert (frame_styles <= set(ran)) == dna and (dna or not frame_styles & set(ran))
    with _open(files, dna, tax=None) as s:
        s.run()
        with pytest.raises(GhostmError, match="taxonomy"):
            s.read_lca(dna)
        assert s.read_lca_stats()["lca_launches"] == 0
