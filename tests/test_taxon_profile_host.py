"""A sample's taxon profile on the host (GhostmTaxonProfileHost; no device):
against the model of taxprofile_cases.py (written from the definitions; no code
shared with taxon_profile.h) on every stage case and on the random calls; the
invariants; every refusal with the outputs untouched; the report of the
hand-written sample as a literal; the struct layouts and the new symbols; the
usage errors; the host arithmetic as a stand-alone program, plain and under
-fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import taxprofile_cases as tp
from ghostm_amd import TAXON_COUNT_DTYPE, GhostmError, native, taxon_profile_host

SRC = os.path.join(os.path.dirname(__file__), "native", "test_taxon_profile.cpp")
CASES = tp.stage_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_model(name):
    parent, node, min_reads = CASES[name]
    want = tp.model(parent, node, min_reads)
    tp.check_invariants(parent, *want, min_reads)
    got = taxon_profile_host(parent, node, min_reads)
    tp.assert_same(got, want, name)
    if name == "single":
        assert got[0].tolist() == [(0, 70, 70, 70)]
    elif name == "chain_one_leaf":
        assert len(got[0]) == 256 and (got[0]["clade_reads"] == 1).all() and got[0]["direct_reads"].sum() == 1
    elif name == "chain_contention":
        assert (got[0]["clade_reads"] == 100000).all() and got[0]["kept_reads"][255] == 100000
    elif name == "chain_spread":   # every node under the floor hands its reads up to the first at 300
        assert got[2]["moved"] > 0 and got[2]["nodes_kept"] < 256
    elif name == "star":
        assert len(got[0]) == 300 and got[0]["kept_reads"][0] == 299 and got[2]["moved"] == 299
    elif name == "binary_full":
        assert len(got[0]) == 2047
    elif name == "small":
        assert got[0].tolist() == tp.SMALL_RECORDS
    elif name.startswith("floor_"):
        s = got[2]
        if min_reads == 1:
            assert s["moved"] == 0 and np.array_equal(got[1], node)
        elif min_reads == s["classified"] + 1:   # everything unclassified, the records still listed
            assert s["kept"] == 0 and s["nodes_kept"] == 0 and (got[1] == tp.NONE).all() and len(got[0]) > 100
        else:
            assert s["kept"] == s["classified"] and s["moved"] > 0


def test_the_floor_cases_straddle_a_clade_count():
    floors = sorted(c[2] for c in tp.floor_cases().values())
    parent, node, _ = next(iter(tp.floor_cases().values()))
    rec = tp.model(parent, node, 1)[0]
    mid = floors[2]
    assert floors[:2] == [1, 2] and floors[3] == mid + 1 and (rec["clade_reads"] == mid).any()
    at = tp.model(parent, node, mid)[2]["nodes_kept"]
    assert tp.model(parent, node, mid + 1)[2]["nodes_kept"] < at


def test_host_equals_the_model_on_random_calls_and_they_are_not_vacuous():
    moved = under = none = 0
    for k, (parent, node, min_reads) in enumerate(tp.random_calls()):
        want = tp.model(parent, node, min_reads)
        tp.check_invariants(parent, *want, min_reads)
        tp.assert_same(taxon_profile_host(parent, node, min_reads), want, ("random", k))
        moved += want[2]["moved"] > 0
        under += want[2]["nodes_kept"] < want[2]["nodes"]
        none += want[2]["classified"] < want[2]["reads"]
    assert moved >= 40 and under >= 60 and none >= 60, (moved, under, none)


def test_final_node_is_optional_and_the_count_query():
    parent, node, min_reads = CASES["random"]
    want = tp.model(parent, node, min_reads)
    rec, final, summary = taxon_profile_host(parent, node, min_reads, with_final=False)
    assert final is None
    tp.assert_same((rec, None, summary), want, "no final")
    rec, _, _ = taxon_profile_host(parent, node, min_reads, cap=len(want[0]) + 5)   # room to spare
    assert np.array_equal(rec, want[0])
    with pytest.raises(GhostmError, match=f"GhostmTaxonProfileHost: cap: {len(want[0])} "):
        taxon_profile_host(parent, node, min_reads, cap=len(want[0]) - 1)


def test_host_refusals():
    tp.check_refusals("GhostmTaxonProfileHost", True)
    with pytest.raises(GhostmError, match="param"):
        taxon_profile_host(tp.SMALL, tp.SMALL_NODES, 0)
    # the taxonomy's own refusals come through
    import readlca_cases as lc
    with pytest.raises(GhostmError, match="GhostmTaxonProfileHost: taxonomy: node 1: a second root"):
        taxon_profile_host(lc.BAD_TREES["two_roots"][0], np.zeros(3, dtype=np.uint32), 1)


def test_the_report_of_the_hand_written_sample():
    rec, _, summary = tp.model(tp.SMALL, tp.SMALL_NODES, tp.SMALL_MIN)
    assert rec.tolist() == tp.SMALL_RECORDS and summary["reads"] == 13
    assert tp.report(tp.SMALL, tp.SMALL_TAXID, rec, tp.SMALL_MIN, 13) == tp.SMALL_REPORT
    assert tp.report(tp.SMALL, tp.SMALL_TAXID, rec[:0], 1, 0) == b""
    assert tp.percent(1, 20000) == "0.01" and tp.percent(2, 3) == "66.67" and tp.percent(0xFFFFFFFF, 0xFFFFFFFF) == "100.00"


def test_struct_layout_and_symbols():
    assert ctypes.sizeof(native.GhostmTaxonCount) == TAXON_COUNT_DTYPE.itemsize == 16
    assert [n for n, _ in native.GhostmTaxonCount._fields_] == list(TAXON_COUNT_DTYPE.names)
    for name, _ in native.GhostmTaxonCount._fields_:
        assert TAXON_COUNT_DTYPE.fields[name][1] == getattr(native.GhostmTaxonCount, name).offset, name
    assert [n for n, _ in native.GhostmTaxonSummary._fields_] == ["reads", "classified", "kept", "moved", "nodes", "nodes_kept"]
    assert [n for n, _ in native.GhostmTaxonProfileStats._fields_] == [
        "seconds_profile", "profile_launches", "profile_reads", "profile_nodes"]
    assert ctypes.sizeof(native.GhostmTaxonSummary) == 48 and ctypes.sizeof(native.GhostmTaxonProfileStats) == 32
    stats = [n for n, _ in native.GhostmStats._fields_]   # GhostmStats keeps its layout
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]
    lib = native.load()
    names = ("TaxonProfileGpu", "GhostmTaxonProfileHost", "GhostmStageTaxonProfileStats", "GhostmSessionSetProfile",
             "GhostmSessionTaxonProfile", "GhostmSessionTaxonProfileFinal", "GhostmSessionTaxonProfileSummary",
             "GhostmSessionTaxonProfileStats")
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ghostm_hip.h")).read()
    for sym in names:
        assert hasattr(lib, sym) and sym in native.SIGNATURES and sym + "(" in header, sym
    for sym in ("GhostmTaxonCount;", "GhostmTaxonSummary;", "GhostmTaxonProfileStats;"):
        assert sym in header, sym


def test_usage_errors_need_no_device(tmp_path):
    """-y 24 / -y 25 without both files, -R out of range: 1 and the usage text,
    no output file, before any device call; aln names search."""
    import cases

    out = str(tmp_path / "o")
    base = [cases.GHOSTM, "search", "-f", "db.fa"]
    for extra in (["-y", "24"], ["-y", "25", "-n", "nodes"], ["-y", "24", "-a", "map"],
                  ["-n", "nodes", "-a", "map", "-R", "0"], ["-n", "nodes", "-a", "map", "-R", "-3"],
                  ["-n", "nodes", "-a", "map", "-R", "x"], ["-n", "nodes", "-a", "map", "-R", "4294967296"]):
        r = subprocess.run(base + extra + ["q.fa", out], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"ghostm (") and b"[-R minReads]" in r.stderr, (extra, r)
        assert not os.path.exists(out)
    for y in ("24", "25"):
        r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", out, "-y", y], capture_output=True)
        assert r.returncode == 0 and b"search" in r.stderr and not os.path.exists(out), r


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_arithmetic_native(flags, tmp_path):
    exe = str(tmp_path / "test_taxon_profile")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
