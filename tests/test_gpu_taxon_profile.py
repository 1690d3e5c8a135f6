"""A sample's taxon profile on the device: the k_taxon_* kernels at the stage
level (TaxonProfileGpu against GhostmTaxonProfileHost, every record, final node
and total equal: the read counts at the wave's and the workgroup's borders
with full and with no aggregation, every tree, the floor at its limits, 150
random calls whole and in batches of three reads, the clean state of the count
arrays after every kind of call, the count query, the refusals, the counters,
the LDS poison build); the session post-pass (Session.taxon_profile) on reads
that fall into two families, as protein and as DNA; -y 24, -y 25 and -R; a
session that does not ask for the profile prints what it printed."""
import ctypes
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
import taxprofile_cases as tp
import test_gpu_read_lca as rl
from ghostm_amd import (TAXON_COUNT_DTYPE, GhostmError, native, set_taxonomy_gpu, stage_read_lca_stats,
                        stage_taxon_profile_stats, taxon_profile, taxon_profile_host)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = rl.POISON_LIB
CASES = tp.stage_cases()
_Env = pc.pr_env
NONE = tp.NONE


def _counted(node, min_reads, want, batches=None, **kw):
    """TaxonProfileGpu on the resident taxonomy, the counters checked against the records"""
    s0 = stage_taxon_profile_stats()
    got = taxon_profile(node, min_reads, **kw)
    s1 = stage_taxon_profile_stats()
    calls = 2 if kw.get("cap") is None else 1   # the count query first
    assert s1["profile_reads"] - s0["profile_reads"] == calls * len(node)
    assert s1["profile_nodes"] - s0["profile_nodes"] == calls * len(want[0])
    if batches is None:
        batches = 1 if len(node) else 0
    assert s1["profile_launches"] - s0["profile_launches"] == calls * batches
    assert (s1["seconds_profile"] > s0["seconds_profile"]) == bool(len(node))
    return got


# ------------------------------------------------------------ stage level
@pytest.mark.parametrize("name", list(CASES))
def test_stage_equals_host_model(name):
    parent, node, min_reads = CASES[name]
    want = taxon_profile_host(parent, node, min_reads)
    tp.check_invariants(parent, *want, min_reads)
    set_taxonomy_gpu(parent)
    tp.assert_same(_counted(node, min_reads, want), want, name)
    if name == "chain_one_leaf":
        assert len(want[0]) == 256
    elif name == "binary_full":
        assert len(want[0]) == len(parent) == 2047
    elif name == "small":
        assert want[0].tolist() == tp.SMALL_RECORDS


def test_stage_random_calls_whole_and_in_batches_of_three():
    calls = tp.random_calls()
    assert len(calls) == 150
    set_taxonomy_gpu(calls[0][0])
    wants = [taxon_profile_host(*c) for c in calls]
    for k, ((_, node, min_reads), want) in enumerate(zip(calls, wants)):
        tp.assert_same(_counted(node, min_reads, want, cap=len(want[0])), want, ("random", k))
    with _Env({"GHOSTM_PROFILE_BATCH_READS": "3"}):
        for k, ((_, node, min_reads), want) in enumerate(zip(calls, wants)):
            got = _counted(node, min_reads, want, batches=(len(node) + 2) // 3, cap=len(want[0]))
            tp.assert_same(got, want, ("batches of three", k))
    # one larger sample cut into many batches, the final nodes gathered batch by batch
    parent, node, min_reads = CASES["random"]
    want = taxon_profile_host(parent, node, min_reads)
    with _Env({"GHOSTM_PROFILE_BATCH_READS": "257"}):
        tp.assert_same(_counted(node, min_reads, want, batches=(len(node) + 256) // 257), want, "batches of 257")


def test_stage_clean_state():
    """Stale counts would show in the next call: two different calls back to
    back, a call after each kind of refused call, a smaller and then a larger
    tree, a call after FreeGpu."""
    parent, node, min_reads = CASES["random"]
    other = tp.sample(parent, 1500, 9)
    set_taxonomy_gpu(parent)
    for nd, m in ((node, min_reads), (other, 1), (node, min_reads), (other, 7)):
        tp.assert_same(taxon_profile(nd, m), taxon_profile_host(parent, nd, m), "back to back")
    want = taxon_profile_host(parent, other, 3)
    bad = node.copy()
    bad[100] = len(parent)
    with pytest.raises(GhostmError, match="TaxonProfileGpu: .*node: read 100:"):   # refused before any launch
        taxon_profile(bad, 3)
    tp.assert_same(taxon_profile(other, 3), want, "after a refused node")
    need = len(taxon_profile_host(parent, node, 3)[0])
    with pytest.raises(GhostmError, match=f"TaxonProfileGpu: .*cap: {need} "):    # refused after the counts
        taxon_profile(node, 3, cap=need - 1)
    tp.assert_same(taxon_profile(other, 3), want, "after a refused cap")
    taxon_profile(node, 3, cap=need)
    small = lc.TREES["binary"]   # a smaller tree, then the larger one again
    folded = np.where(other == NONE, NONE, other % len(small)).astype(np.uint32)
    set_taxonomy_gpu(small)
    tp.assert_same(taxon_profile(folded, 2), taxon_profile_host(small, folded, 2), "the smaller tree")
    with pytest.raises(GhostmError, match="node: read"):   # the larger tree's nodes are out of range now
        taxon_profile(node, 2)
    set_taxonomy_gpu(parent)
    tp.assert_same(taxon_profile(other, 3), want, "the larger tree again")
    with pytest.raises(GhostmError, match="SetTaxonomyGpu: taxonomy: node 1: a second root"):
        set_taxonomy_gpu(lc.BAD_TREES["two_roots"][0])   # a refused taxonomy keeps the resident one and its arrays
    tp.assert_same(taxon_profile(other, 3), want, "after a refused taxonomy")
    assert native.load().FreeGpu() == 0
    with pytest.raises(GhostmError, match="TaxonProfileGpu: .*taxonomy: "):
        taxon_profile(other, 3)
    set_taxonomy_gpu(parent)
    tp.assert_same(taxon_profile(other, 3), want, "after FreeGpu")


def test_stage_final_node_count_query_and_cap():
    parent, node, min_reads = CASES["random"]
    want = taxon_profile_host(parent, node, min_reads)
    need = len(want[0])
    set_taxonomy_gpu(parent)
    rec, final, summary = taxon_profile(node, min_reads, with_final=False)
    assert final is None
    tp.assert_same((rec, None, summary), want, "final_node NULL")
    tp.assert_same(taxon_profile(node, min_reads, with_final=True), want, "final_node given")
    assert want[2]["moved"] > 0 and (want[1] != node).any()
    lib = native.load()
    nout = ctypes.c_size_t(tp.POISON)
    assert tp.raw_call(lib.TaxonProfileGpu, None, node, min_reads, 0, None, nout, None, None) == 0
    assert nout.value == need
    out = np.full(4 * need, tp.POISON, dtype=np.uint32).view(TAXON_COUNT_DTYPE)
    nout = ctypes.c_size_t(tp.POISON)
    assert tp.raw_call(lib.TaxonProfileGpu, None, node, min_reads, need - 1, out, nout, None, None) == 1
    assert f"cap: {need} " in native.last_error() and nout.value == tp.POISON and (out.view(np.uint32) == tp.POISON).all()
    assert tp.raw_call(lib.TaxonProfileGpu, None, node, min_reads, need, out, nout, None, None) == 0
    assert nout.value == need and np.array_equal(out, want[0])


def test_stage_refusals_and_counters():
    """Every reason on the device entry point, the outputs untouched; a refused
    call counts no reads and no nodes, and one refused before the counts
    launches nothing."""
    set_taxonomy_gpu(tp.SMALL)
    want = taxon_profile_host(tp.SMALL, tp.SMALL_NODES, tp.SMALL_MIN)
    tp.assert_same(taxon_profile(tp.SMALL_NODES, tp.SMALL_MIN), want, "small")
    s0 = stage_taxon_profile_stats()
    l0 = stage_read_lca_stats()
    with pytest.raises(GhostmError, match="param"):
        taxon_profile(tp.SMALL_NODES, 0)
    bad = tp.SMALL_NODES.copy()
    bad[3] = 10
    with pytest.raises(GhostmError, match="node: read 3:"):
        taxon_profile(bad, 1)
    assert stage_taxon_profile_stats() == s0
    tp.check_refusals("TaxonProfileGpu", False)   # its "cap" refusals and its count query launch
    s1 = stage_taxon_profile_stats()
    assert s1["profile_reads"] - s0["profile_reads"] == len(tp.SMALL_NODES)    # the count query alone
    assert s1["profile_nodes"] - s0["profile_nodes"] == len(tp.SMALL_RECORDS)
    assert stage_read_lca_stats() == l0
    tp.assert_same(taxon_profile(tp.SMALL_NODES, tp.SMALL_MIN), want, "after the refusals")


@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_stage_under_lds_poison(pattern):
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "taxprofile_poison_child.py")], capture_output=True, text=True,
                       timeout=60, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])


# ------------------------------------------------------------ session level
W, STEP = rl.W, rl.STEP
TAXID, PARENT = rl.TAXID, rl.PARENT


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """test_gpu_read_lca.py's database, taxonomy and two-gene read, and beside
    that read one of gene C alone (the other family), one of gene A alone and
    one of noise: three reads with a taxon in two families."""
    tmp = str(tmp_path_factory.mktemp("taxprofile"))
    subjects, prot, _ = rl._inputs()
    r = random.Random(20270104)
    gene = {name.split()[0]: seq for name, seq in subjects}
    prot = prot + [("readC", fc.rand_prot(r, 20) + fc.mutate(r, gene["geneC"], 0.03) + fc.rand_prot(r, 20)),
                   ("readA", fc.mutate(r, gene["geneA"], 0.02)), ("noise", fc.rand_prot(r, 200))]
    dna = [(name, fc.back_translate(seq)) for name, seq in prot]
    out = dict(tmp=tmp, db=os.path.join(tmp, "db.fa"), prot=prot, dna=dna, prot_fa=os.path.join(tmp, "prot.fa"),
               dna_fa=os.path.join(tmp, "dna.fa"), nodes=os.path.join(tmp, "nodes.dmp"), map=os.path.join(tmp, "map.tsv"))
    for path, records in ((out["db"], subjects), (out["prot_fa"], prot), (out["dna_fa"], dna)):
        with open(path, "w") as f:
            for name, seq in records:
                f.write(f">{name}\n{seq}\n")
    with open(out["nodes"], "w") as f:
        for t, p in rl.NODES:
            f.write(f"{t}\t|\t{p}\t|\tno rank\t|\n")
    with open(out["map"], "w") as f:
        for name, t in rl.SUBJECT_TAXID.items():
            f.write(f"{name}\t{t}\n")
    out["subject_node"] = np.array([list(TAXID).index(rl.SUBJECT_TAXID[n.split()[0]]) for n, _ in subjects], dtype=np.uint32)
    return out


def _profile(files, dna, tmp_path):
    frame, y_paths, y_lca, y_prof = (True, "13", "23", "25") if dna else (False, "12", "22", "24")
    with rl._open(files, dna, y=y_paths) as s:
        s.run()
        assert s.taxon_profile_stats()["profile_launches"] == 0   # the path styles ask for no profile
        lca = s.read_lca(frame)
        total = len(lca)
        assert total >= 3 and lca["node"][0] == rl.FAMILY   # the two-gene read is the family's
        lca_stats = s.read_lca_stats()
        got = s.taxon_profile(frame)
        want = taxon_profile_host(PARENT, lca["node"], 1)
        tp.assert_same(got, want, "floor 1")
        assert got[2]["reads"] == total and got[2]["moved"] == 0 and got[2]["classified"] >= 3
        st = s.taxon_profile_stats()
        assert st["profile_launches"] == 1 and st["profile_reads"] == total and st["profile_nodes"] == len(want[0])
        s.taxon_profile(frame)
        s.set_profile(1)   # no change
        s.taxon_profile(frame)
        assert s.taxon_profile_stats() == st   # kept: nothing launched
        text1 = tp.report(PARENT, TAXID, got[0], 1, total)
        s.set_profile(2)   # a change drops the profile and only the profile
        got2 = s.taxon_profile(frame)
        tp.assert_same(got2, taxon_profile_host(PARENT, lca["node"], 2), "floor 2")
        assert s.taxon_profile_stats()["profile_launches"] == 2 and s.read_lca_stats() == lca_stats
        assert got2[2]["moved"] > 0 and got2[2]["nodes_kept"] < got2[2]["nodes"], got2   # a clade is pruned
        text2 = tp.report(PARENT, TAXID, got2[0], 2, total)
        assert text1 != text2 and len(text2.splitlines()) < len(text1.splitlines())
        s.set_lca(100, 60)   # what drops the assignment drops the profile
        lca60 = s.read_lca(frame)
        tp.assert_same(s.taxon_profile(frame), taxon_profile_host(PARENT, lca60["node"], 2), "after set_lca")
        assert s.taxon_profile_stats()["profile_launches"] == 3
        with pytest.raises(GhostmError, match="param"):
            s.set_profile(0)
        if not dna:
            with pytest.raises(GhostmError, match="tiled"):   # refused where read_lca(True) is
                s.taxon_profile(True)
    with rl._open(files, dna, y=y_prof) as s:
        s.run()
        assert s.output() == text1 and text1.count(b"\n") >= 4
        assert s.taxon_profile_stats()["profile_launches"] == 1
    with rl._open(files, dna, y=y_prof, tax="files") as s:
        s.set_profile(2)
        s.run()
        assert s.output() == text2
    for floor, text in ((1, text1), (2, text2)):   # the command form
        out_path = str(tmp_path / f"profile{floor}.out")
        cmd = [cases.GHOSTM, "search", "-q", "d" if dna else "p", "-w", str(3 * W if dna else W), "-T", str(STEP), "-y", y_prof,
               "-b", "3", "-D", "0", "-g", "-n", files["nodes"], "-a", files["map"], "-R", str(floor), "-f", files["db"],
               files["dna_fa" if dna else "prot_fa"], out_path]
        r = subprocess.run(cmd, capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(out_path, "rb").read() == text, floor
    # a session that does not ask for the profile prints what it printed: -y 22 / -y 23 against its own formatter
    with rl._open(files, dna, y=y_lca) as s:
        s.set_profile(7)
        s.run()
        text = s.output()
        names = [line.split(b"\t")[0].decode() for line in text.splitlines()]
        assert text == rl._want_text(names, s.read_lca(frame)) and len(names) == total
        assert s.taxon_profile_stats()["profile_launches"] == 0


def test_session_protein(files, tmp_path):
    _profile(files, False, tmp_path)
    with rl._open(files, False, y="25") as s:   # -y 25 on a protein set: the error -y 13 gives
        with pytest.raises(GhostmError, match="tiled"):
            s.run()


def test_session_dna(files, tmp_path):
    _profile(files, True, tmp_path)


def test_no_hits_and_no_taxonomy(files):
    """A run without hits writes an empty file; without a taxonomy the style is
    refused as -y 22 is; -y 0 does not hear of the floor."""
    with rl._open(files, False, y="24") as s:
        s.set_queries([fc.rand_prot(random.Random(5), 150)], ["nothing"], width=W, dna=False, tile_step=STEP)
        s.run()
        assert len(s.hits()) == 0 and s.output() == b""
        rec, final, summary = s.taxon_profile(False)
        assert len(rec) == 0 and len(final) == 0 and summary == dict.fromkeys(summary, 0)
    with rl._open(files, False, y="24", tax=None) as s:
        with pytest.raises(GhostmError, match="taxonomy"):
            s.run()
    outs = []
    for floor in (None, 9):
        with rl._open(files, False, y="0") as s:
            if floor:
                s.set_profile(floor)
            s.run()
            stats = {k: v for k, v in s.stats().items() if not k.startswith("seconds")}
            outs.append((s.output(), s.hits().tobytes(), stats, s.taxon_profile_stats()["profile_launches"]))
    assert outs[0] == outs[1] and outs[0][3] == 0 and len(outs[0][0]) > 0
