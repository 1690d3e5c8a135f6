"""The read-level subject pile-up on the host (GhostmReadPileupHost, no device):
against the Python model of the contract (readpileup_cases.py) on the hand-made
band and frame paths of both strand layouts, on the paths GhostmBandAlignHost /
GhostmFrameAlignHost make, and on the tile-edge shapes; against
GhostmPathPileupHost on single-tile sources; every refusal with the outputs
untouched; the struct layouts; the span rule as a stand-alone program, plain and
under -fsanitize=address,undefined; and the point of the feature on the model
alone: a 300-letter read piles up on more than 127 positions."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import band_cases as bc
import pathrows_cases as pr
import pileup_cases as pc
import readpileup_cases as rp
import readrows_cases as rc
from ghostm_amd import (BAND_SOURCE_DTYPE, READ_PILEUP_DTYPE, SUBJECT_PILEUP_DTYPE, native, path_pileup_host,
                        read_pileup_host)

SRC = os.path.join(os.path.dirname(__file__), "native", "test_read_pileup_span.cpp")
SETS = rp.stage_sets()


@pytest.mark.parametrize("name,build", SETS, ids=[n for n, _ in SETS])
def test_host_equals_the_model(name, build):
    """All hits, one hit, no hit; with and without shifts and the profile."""
    rs = build()
    call = rp.host_call(native.load(), rs)
    for count in (None, 1, 0):
        want = rp.check_against_model(call, rs, (name, count), count)
        assert int(want[0].sum()) > 0 or count == 0
        if count == 0:
            assert (want[2] == 255).all() and int(want[4].sum()) == 0
    full = rp.model(rs)
    cols, shifts = rp.charged_columns(rs.rec, rs.ops)
    assert int(full[0].sum()) == cols and int(full[3].sum()) == shifts
    if name.startswith("hand_frame") or name.startswith("truth"):
        assert shifts > 0
    # the Python wrapper returns the same arrays
    got = read_pileup_host(rs.qseq, rs.W, rs.db, rs.src, rs.rec, rs.ops, rs.step, rs.frame, profile=True)
    rp.assert_same(got, full, "wrapper")
    assert read_pileup_host(rs.qseq, rs.W, rs.db, rs.src, rs.rec, rs.ops, rs.step, rs.frame, shifts=False)[3:] == \
        (None, None)


def test_host_on_the_tile_edge_shapes():
    """The shapes the device is run on at tiles of 32 positions: here the host
    model and the Python model agree on them and they show what they are for."""
    lib = native.load()
    for strand in (0, 1):
        for name, rs in rp.edge_sets(strand).items():
            want = rp.model(rs)
            rp.assert_same(rp.pileup_via(rp.host_call(lib, rs), rs), want, name)
            rp.expected_edges(name, want)
    sets = rp.edge_sets(0)
    for mode in ("frame", "band"):
        a, b = rp.model(sets[mode + "_mixed"]), rp.model(sets[mode + "_mixed_reversed"])
        rp.assert_same(a, b, "order")


@pytest.mark.parametrize("L", [24, 127])
def test_single_tile_sources_equal_the_tile_pileup(L, data_root):
    """Band mode with every record its own single-tile source is the tile
    pile-up: GhostmPathPileupHost's arrays on the indel fixture's tile paths."""
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, L)
    nq, _, qseq, dbseq, pos = chunk
    src = np.zeros(len(qid), dtype=BAND_SOURCE_DTYPE)
    src["first_record"], src["stride"], src["tiles"], src["letters"] = qid, 1, 1, L
    want = path_pileup_host(qseq, L, dbseq, qid, rec, ops, profile=True)
    got = read_pileup_host(qseq, L, dbseq, src, rec, ops, L, frame=False, profile=True)
    assert int(want[0].sum()) > 0 and int(want[3][:, 26].sum()) > 0
    for k, name in ((0, "depth"), (1, "identities"), (2, "consensus")):
        assert np.array_equal(got[k], want[k]), name
    assert np.array_equal(got[4], want[3]) and int(got[3].sum()) == 0
    # the hand-made tile paths and the edge shapes of the tile pile-up's own tests
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    sets = dict(pc.edge_cases(nq, L, len(dbseq)), hand=pr.hand_paths(nq, L, len(dbseq)))
    for name, (q, r, o) in sets.items():
        src = np.zeros(len(q), dtype=BAND_SOURCE_DTYPE)
        src["first_record"], src["stride"], src["tiles"], src["letters"] = q, 1, 1, L
        want = path_pileup_host(qseq, L, dbseq, q, r, o, profile=True)
        got = read_pileup_host(qseq, L, dbseq, src, r, o, L, frame=False, profile=True)
        for k in range(3):
            assert np.array_equal(got[k], want[k]), (name, k)
        assert np.array_equal(got[4], want[3]), name


@pytest.mark.parametrize("build", [rc.hand_band_set, lambda: rc.hand_frame_set(0)], ids=["band", "frame"])
def test_host_refusals(build):
    rs = build()
    rp.check_refusals(rp.host_call(native.load(), rs), rs, gpu=False)


def test_struct_layout():
    assert ctypes.sizeof(native.GhostmSubjectReadPileup) == READ_PILEUP_DTYPE.itemsize == 48
    for name, _ in native.GhostmSubjectReadPileup._fields_:
        f = getattr(native.GhostmSubjectReadPileup, name)
        assert READ_PILEUP_DTYPE.fields[name][1] == f.offset and READ_PILEUP_DTYPE.fields[name][0].itemsize == f.size, name
    assert list(READ_PILEUP_DTYPE.names[:7]) == list(SUBJECT_PILEUP_DTYPE.names)
    for name in SUBJECT_PILEUP_DTYPE.names:
        assert READ_PILEUP_DTYPE.fields[name][1] == SUBJECT_PILEUP_DTYPE.fields[name][1]
    assert [n for n, _ in native.GhostmReadPileupStats._fields_] == [
        "seconds_read_pileup", "read_pileup_launches", "read_pileup_windows", "read_pileup_parts", "read_pileup_columns",
        "read_pileup_shifts"]
    assert ctypes.sizeof(native.GhostmReadPileupStats) == 48
    stats = [n for n, _ in native.GhostmStats._fields_]   # GhostmStats keeps its layout
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_span_rule_native(flags, tmp_path):
    exe = str(tmp_path / "test_read_pileup_span")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout


def planted_long_read():
    """A subject of 300 residues and a read that matches it end to end at a 4 %
    substitution rate, as a band_cases stage case on diagonal 0."""
    rnd = random.Random(20261102)
    subject = bc.rand_seq(rnd, 300)
    return bc.Case(127, 64, 1, 31, [bc.mutate(rnd, subject, 0.04)], [subject], [(0, 0, 0)]), subject


def test_a_long_read_covers_more_than_one_tile():
    """The point of the feature on the model alone: the band path of a 300-letter
    read covers at least 254 positions (two full tiles' worth); a tile path
    covers at most 127 by construction."""
    case, subject = planted_long_read()
    rs = rc.made_band_set(case)
    depth = rp.model(rs)[0]
    assert int((depth > 0).sum()) >= 254
    rp.assert_same(rp.pileup_via(rp.host_call(native.load(), rs), rs), rp.model(rs), "long read")
