"""The per-read taxonomic assignment on the host (GhostmReadLcaHost,
GhostmTaxonomyDepths; no device): against the brute-force model of
readlca_cases.py (ancestor sets and a counter per node; no code shared with
read_lca.h) on the small shapes, every tree, the reads at the kernel's class
borders, one call that mixes them and a few hundred random reads; that the
random reads exercise what they are for; every refusal with the outputs
untouched; the depths and their refusals; the struct layouts and the new
symbols; the host arithmetic and the parsers as a stand-alone program, plain
and under -fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import readlca_cases as lc
from ghostm_amd import LCA_HIT_DTYPE, LCA_OUT_DTYPE, GhostmError, native, read_lca_host, taxonomy_depths

SRC = os.path.join(os.path.dirname(__file__), "native", "test_read_lca.cpp")
SHAPES = lc.shape_cases()
TREE_CASES = lc.tree_cases()


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_equals_the_model_on_the_shapes(name):
    case = SHAPES[name]
    want = lc.model(*case)
    lc.expected_shapes(name, want)
    lc.assert_same(read_lca_host(*case), want, name)


@pytest.mark.parametrize("name", list(TREE_CASES))
def test_host_equals_the_model_on_the_trees(name):
    case = TREE_CASES[name]
    want = lc.model(*case)
    lc.assert_same(read_lca_host(*case), want, name)
    if name == "single":
        assert (want["node"][want["votes"] > 0] == 0).all() and (want["depth"] == 0).all()
    elif name == "star_leaves":   # seventy leaves: only the root holds them
        assert want[0].tolist() == (0, 0, 70, 70, 0, 70, 0, 50)
    elif name == "chain_ends":   # thr 2 of 3: the deepest node with two votes below or at it
        assert want[0].tolist() == (254, 254, 3, 2, 3, 3, 0, 50)
    elif name == "chain":
        assert want["depth"].max() > 100


@pytest.mark.parametrize("n", lc.SIZES)
def test_host_equals_the_model_at_the_class_borders(n):
    case = lc.sized_read(n)
    assert lc.candidates_of(case) == n and len(case[2]) > n and case[2]["score"][0] == 0
    want = lc.model(*case)
    assert want["candidates"][0] == n and want["votes"][0] > n // 8
    lc.assert_same(read_lca_host(*case), want, n)


def test_host_equals_the_model_on_the_mixed_call():
    case = lc.mixed_call()
    lc.assert_same(read_lca_host(*case), lc.model(*case), "mixed")


def test_host_equals_the_model_on_random_reads_and_they_are_not_vacuous():
    par = [int(p) for p in lc.RANDOM_TREE]
    has_child = np.zeros(len(par), dtype=bool)
    for i, p in enumerate(par):
        if p != i:
            has_child[p] = True
    root = next(i for i, p in enumerate(par) if p == i)
    voting = split = inner = unmapped = failed = 0
    for k, case in enumerate(lc.random_calls(150)):
        info = {}
        want = lc.model(*case, info=info)
        lc.assert_same(read_lca_host(*case), want, ("random", k))
        at60 = lc.model(*case[:4], 60)
        for r in np.flatnonzero(want["votes"] > 0):
            voting += 1
            split += at60["node"][r] != at60["lca"][r]
            inner += at60["node"][r] != root and has_child[at60["node"][r]]
            unmapped += want["unmapped"][r] > 0
            failed += info["failed"][r] > 0
    assert voting >= 250, voting
    assert 5 * split >= voting and 5 * inner >= voting and 10 * unmapped >= voting and 10 * failed >= voting, (
        voting, split, inner, unmapped, failed)


def test_the_record_does_not_depend_on_the_order_of_the_hits():
    parent, rb, hits, top, sup = lc.sized_read(300, seed=3)
    want = read_lca_host(parent, rb, hits, top, sup)
    rnd = np.random.default_rng(20261206)
    for _ in range(3):
        lc.assert_same(read_lca_host(parent, rb, hits[rnd.permutation(len(hits))], top, sup), want, "shuffled")


def test_host_refusals():
    lc.check_refusals("GhostmReadLcaHost", True)
    with pytest.raises(GhostmError, match="param"):
        read_lca_host(*SHAPES["one_hit"][:3], support_pct=50)
    # the taxonomy's own refusals come through
    case = SHAPES["one_hit"]
    out = np.full(8, 0xC3C3C3C3, dtype=np.uint32).view(LCA_OUT_DTYPE)
    with pytest.raises(GhostmError, match="taxonomy: node 1: a second root"):
        read_lca_host(lc.BAD_TREES["two_roots"][0], *case[1:], out=out)
    assert (out.view(np.uint32) == 0xC3C3C3C3).all()


def test_taxonomy_depths_and_its_refusals():
    for name, parent in lc.TREES.items():
        assert taxonomy_depths(parent).tolist() == lc.depths(parent), name
    assert int(taxonomy_depths(lc.TREES["chain"]).max()) == 255
    assert int(taxonomy_depths(lc.TREES["binary"]).max()) == 10
    assert 20 <= int(taxonomy_depths(lc.RANDOM_TREE).max()) <= 255
    par = lc.RANDOM_TREE
    assert (par[np.arange(len(par))] > np.arange(len(par))).sum() > 1000   # parents above their children
    for name, (parent, node) in lc.BAD_TREES.items():
        with pytest.raises(GhostmError, match="GhostmTaxonomyDepths: taxonomy: ") as e:
            taxonomy_depths(parent)
        if node is not None:
            assert f"node {node}:" in str(e.value), (name, str(e.value))
    with pytest.raises(GhostmError, match="taxonomy"):
        taxonomy_depths(np.zeros(0, dtype=np.uint32))
    lib = native.load()
    assert lib.GhostmTaxonomyDepths(3, None, None) == 1 and "null: " in native.last_error()
    one = np.zeros(1, dtype=np.uint32)
    assert lib.GhostmTaxonomyDepths(1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None) == 1
    assert "null: " in native.last_error()


def test_struct_layout_and_symbols():
    assert ctypes.sizeof(native.GhostmLcaHit) == LCA_HIT_DTYPE.itemsize == 16
    assert ctypes.sizeof(native.GhostmLcaOut) == LCA_OUT_DTYPE.itemsize == 32
    for struct, dtype in ((native.GhostmLcaHit, LCA_HIT_DTYPE), (native.GhostmLcaOut, LCA_OUT_DTYPE)):
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name
    assert [n for n, _ in native.GhostmReadLcaStats._fields_] == [
        "seconds_lca", "lca_launches", "lca_reads", "lca_hits", "lca_votes", "lca_assigned"]
    assert ctypes.sizeof(native.GhostmReadLcaStats) == 48 and ctypes.sizeof(native.GhostmTaxonomyInfo) == 32
    stats = [n for n, _ in native.GhostmStats._fields_]   # GhostmStats keeps its layout
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]
    lib = native.load()
    names = ("SetTaxonomyGpu", "GhostmTaxonomyDepths", "ReadLcaGpu", "GhostmReadLcaHost", "GhostmStageReadLcaStats",
             "GhostmSessionSetTaxonomy", "GhostmSessionSetTaxonomyFiles", "GhostmSessionTaxonomyInfo",
             "GhostmSessionSetLca", "GhostmSessionReadLca", "GhostmSessionReadLcaBegin", "GhostmSessionReadLcaStats")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ghostm_hip.h")).read()
    for sym in names:
        assert hasattr(lib, sym) and sym in native.SIGNATURES and sym + "(" in header, sym
    for sym in ("GhostmLcaHit;", "GhostmLcaOut;", "GhostmReadLcaStats;", "GhostmTaxonomyInfo;"):
        assert sym in header, sym


def test_usage_errors_need_no_device(tmp_path):
    """-y 22 / -y 23 without both files, one file without the other, -p and -P
    out of range: 1 and the usage text, no output file, before any device call;
    aln names search."""
    import cases

    out = str(tmp_path / "o")
    base = [cases.GHOSTM, "search", "-f", "db.fa"]
    for extra in (["-y", "22"], ["-y", "23", "-n", "nodes"], ["-y", "22", "-a", "map"], ["-n", "nodes"], ["-a", "map"],
                  ["-n", "nodes", "-a", "map", "-p", "101"], ["-n", "nodes", "-a", "map", "-p", "-1"],
                  ["-n", "nodes", "-a", "map", "-P", "50"], ["-n", "nodes", "-a", "map", "-P", "101"],
                  ["-n", "nodes", "-a", "map", "-P", "x"]):
        r = subprocess.run(base + extra + ["q.fa", out], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"ghostm (") and b"\nsearch: " in r.stderr, (extra, r)   # the usage text only
        assert not os.path.exists(out)
    for y in ("22", "23"):
        r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", out, "-y", y], capture_output=True)
        assert r.returncode == 0 and b"search" in r.stderr and not os.path.exists(out), r


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_arithmetic_native(flags, tmp_path):
    exe = str(tmp_path / "test_read_lca")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
