"""The mate-pair join on the host (GhostmPairJoinHost; no device): against the
matrix model of pair_cases.py (no code shared with pair_join.h) on the small
shapes, the pairs at the kernel's class borders, one call that mixes them and a
few hundred random pairs; that the random pairs exercise what they are for;
every refusal with the outputs untouched; the struct layouts and the new
symbols; and the composed example, the join followed by the assignment with the
pairs as reads, without a device."""
import ctypes
import os

import numpy as np
import pytest

import pair_cases as pc
from ghostm_amd import (LCA_HIT_DTYPE, PAIR_HIT_DTYPE, PAIR_OUT_DTYPE, GhostmError, native, pair_join_host,
                        read_lca_host)

SHAPES = pc.shape_cases()


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_equals_the_model_on_the_shapes(name):
    case = SHAPES[name]
    want = pc.model(*case)
    pc.expected_shapes(name, want)
    pc.assert_same(pair_join_host(*case), want, name)


@pytest.mark.parametrize("n", pc.SIZES)
def test_host_equals_the_model_at_the_class_borders(n):
    case = pc.sized_pair(n)
    assert len(case[2]) == n
    info = {}
    want = pc.model(*case, info=info)
    assert info["joined"] > n // 8 and info["taken"] > n // 16 and want[2]["mates"][0] == 3, info
    pc.assert_same(pair_join_host(*case), want, n)


def test_host_equals_the_model_on_the_mixed_call():
    case = pc.mixed_call()
    want = pc.model(*case)
    assert sorted(set(want[2]["mates"].tolist())) == [0, 1, 2, 3]
    pc.assert_same(pair_join_host(*case), want, "mixed")


def test_host_equals_the_model_on_random_pairs_and_they_are_not_vacuous():
    total = {"joined": 0, "taken": 0, "ties": 0, "discordant": 0}
    shared = unjoined = npairs = 0
    for k, case in enumerate(pc.random_calls(150)):
        info = {}
        want = pc.model(*case, info=info)
        pc.assert_same(pair_join_host(*case), want, ("random", k))
        for key in total:
            total[key] += info[key]
        npairs += len(want[2])
        shared += info["joined"] - info["taken"]          # candidates that chose a hit another one chose too
        unjoined += int(((want[2]["mates"] == 3) & (want[2]["joined"] == 0)).sum())
    assert npairs >= 300, npairs
    assert min(total.values()) > 0 and shared > 0 and unjoined > 0, (total, shared, unjoined)
    assert total["joined"] >= 500 and total["taken"] >= 300 and total["ties"] >= 50 and total["discordant"] >= 500, total


def test_hits_outside_every_pair_are_not_written():
    pb, off, h, max_span, orient = SHAPES["joined"]
    outer = np.concatenate([h[:1], h, h[1:]])
    outs = pc.filled_outputs(len(outer), 1)
    got = pair_join_host(pb + 1, off, outer, max_span, orient, out=outs)
    want = pc.model(pb, off, h, max_span, orient)
    assert np.array_equal(got[0][1:3], want[0]) and got[1][1:3].tolist() == [2, 1] and np.array_equal(got[2], want[2])
    for k in (0, 3):
        assert (got[0][k:k + 1].view(np.uint32) == pc.FILL).all() and got[1][k] == pc.FILL


def test_host_refusals():
    pc.check_refusals("GhostmPairJoinHost")
    with pytest.raises(GhostmError, match="GhostmPairJoinHost: param: max_span"):
        pair_join_host(*SHAPES["joined"][:3], max_span=0)


def test_struct_layout_and_symbols():
    assert ctypes.sizeof(native.GhostmPairHit) == PAIR_HIT_DTYPE.itemsize == 32
    assert ctypes.sizeof(native.GhostmPairOut) == PAIR_OUT_DTYPE.itemsize == 16
    for struct, dtype in ((native.GhostmPairHit, PAIR_HIT_DTYPE), (native.GhostmPairOut, PAIR_OUT_DTYPE)):
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name
    assert [n for n, _ in native.GhostmPairJoinStats._fields_] == [
        "seconds_pair", "pair_launches", "pair_pairs", "pair_hits", "pair_joined", "pair_taken"]
    assert ctypes.sizeof(native.GhostmPairJoinStats) == 48
    stats = [n for n, _ in native.GhostmStats._fields_]   # GhostmStats keeps its layout
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]
    lib = native.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ghostm_hip.h")).read()
    for sym in ("PairJoinGpu", "GhostmPairJoinHost", "GhostmStagePairJoinStats", "GhostmSessionSetMates",
                "GhostmSessionSetQueriesFastaMatesTiled", "GhostmSessionPairJoin", "GhostmSessionPairJoinPairs",
                "GhostmSessionPairLca", "GhostmSessionPairJoinStats"):
        assert hasattr(lib, sym) and sym in native.SIGNATURES and sym + "(" in header, sym
    for sym in ("GhostmPairHit;", "GhostmPairOut;", "GhostmPairJoinStats;"):
        assert sym in header, sym


# The composed example: subjects A and B under different leaves of one parent.
ROOT, PARENT, LEAF_A, LEAF_B = range(4)
TREE = np.array([ROOT, ROOT, PARENT, PARENT], dtype=np.uint32)
SUB_A, SUB_B = 11, 12


def composed(mate2_s_lo):
    rows1 = [(SUB_A, LEAF_A, 100, 0, 49, 1000, 1049, 0), (SUB_B, LEAF_B, 100, 0, 49, 400, 449, 0)]
    rows2 = [(SUB_A, LEAF_A, 80, 0, 49, mate2_s_lo, mate2_s_lo + 49, 1)]
    return pc.one_pair(rows1, rows2, offset=50, max_span=400, orient=1)


def test_the_pair_is_assigned_where_its_mates_are_not():
    pb, off, h, max_span, orient = composed(1350)   # span 1000 .. 1399: exactly max_span
    # unpaired: every mate a read of its own
    alone = np.zeros(len(h), dtype=LCA_HIT_DTYPE)
    for f in LCA_HIT_DTYPE.names:
        alone[f] = h[f]
    got = read_lca_host(TREE, pb, alone, top_pct=10, support_pct=100)
    assert got["node"].tolist() == [PARENT, LEAF_A] and got["votes"].tolist() == [2, 1]
    # paired: A at 180 and B at 100; B fails the score test, 100 * 100 < 90 * 180
    cand, partner, pairs = pair_join_host(pb, off, h, max_span, orient)
    assert [tuple(int(v) for v in c) for c in cand] == [(LEAF_A, 180, 0, 99), (LEAF_B, 100, 0, 49), (0, 0, 0, 0)]
    assert partner.tolist() == [2, pc.NONE, 0] and pairs[0].tolist() == (1, 3, 180, 400)
    pair = read_lca_host(TREE, pb[[0, 2]], cand, top_pct=10, support_pct=100)
    assert (pair["node"][0], pair["votes"][0], pair["candidates"][0], pair["best_score"][0]) == (LEAF_A, 1, 2, 180)
    # one residue further the mates no longer join, and the pair's three candidates give the parent again
    pb, off, h, max_span, orient = composed(1351)
    cand, partner, pairs = pair_join_host(pb, off, h, max_span, orient)
    assert pairs[0].tolist() == (0, 3, 100, 0) and (partner == pc.NONE).all()
    assert [tuple(int(v) for v in c) for c in cand] == [(LEAF_A, 100, 0, 49), (LEAF_B, 100, 0, 49), (LEAF_A, 80, 50, 99)]
    pair = read_lca_host(TREE, pb[[0, 2]], cand, top_pct=10, support_pct=100)
    assert (pair["node"][0], pair["votes"][0], pair["lca"][0]) == (PARENT, 3, PARENT)


def test_session_calls_refuse_a_null_session():
    lib = native.load()
    bad = ctypes.c_size_t(-1).value
    assert lib.GhostmSessionSetMates(None, 1, 1000) == 1 and "null session" in native.last_error()
    assert lib.GhostmSessionSetQueriesFastaMatesTiled(None, b"a.fa", b"b.fa", 127, 0, 0, 0, 64, None) == 1
    assert lib.GhostmSessionPairJoin(None, 0, None, None, 0) == bad and "null session" in native.last_error()
    assert lib.GhostmSessionPairJoinPairs(None, 0, None, None, None, 0) == bad
    assert lib.GhostmSessionPairLca(None, 0, None, 0) == bad
    st = native.GhostmPairJoinStats()
    assert lib.GhostmSessionPairJoinStats(None, ctypes.byref(st), ctypes.sizeof(st)) == 0
    assert lib.GhostmStagePairJoinStats(None, 48) == 0


def test_usage_errors_need_no_device(tmp_path):
    """-j, -J and -I without -T, both layouts at once, -y 26 without mates or
    without a taxonomy: 1 and the usage text, no output file, before any device
    call; aln names search."""
    import subprocess

    import cases

    out = str(tmp_path / "o")
    base = [cases.GHOSTM, "search", "-f", "db.fa"]
    tax = ["-n", "nodes", "-a", "map"]
    for extra in (["-j"], ["-J"], ["-I", "500"], ["-T", "64", "-j", "-J"], ["-T", "64", "-I", "500"],
                  ["-T", "64", "-j", "-I", "0"], ["-T", "64", "-y", "26"] + tax, ["-T", "64", "-j", "-y", "27"]):
        r = subprocess.run(base + extra + ["q.fa", out], capture_output=True)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"ghostm (") and b"\nsearch: " in r.stderr, (extra, r)
        assert not os.path.exists(out)
    for y in ("26", "27"):
        r = subprocess.run([cases.GHOSTM, "aln", "-i", "x", "-d", "y", "-o", out, "-y", y], capture_output=True)
        assert r.returncode == 0 and b"search" in r.stderr and b"mates" in r.stderr and not os.path.exists(out), r
