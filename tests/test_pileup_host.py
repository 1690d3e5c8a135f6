"""The subject pile-up's host model (GhostmPathPileupHost, no device) against
the numpy model of tests/pileup_cases.py: the indel fixture's paths at L = 24,
75 and 127, the hand-made paths, the shapes at the tile edges, the struct
layout and the refused calls. The device side is test_gpu_pileup.py."""
import ctypes

import numpy as np
import pytest

import pathrows_cases as pr
import pileup_cases as pc
from ghostm_amd import SUBJECT_PILEUP_DTYPE, consensus_text, native, path_pileup_host


@pytest.mark.parametrize("L", [24, 75, 127])
def test_host_equals_numpy_model_on_the_fixture(L, data_root):
    d, chunk, M, qid, rec, ops = pr.fixture_paths(data_root, L)
    call = pc.host_call(native.load(), chunk)
    for count in (len(qid), 1, 0):
        want = pc.check_against_model(call, chunk, qid[:count], rec[:count], ops, count)
        assert int(want[0].sum()) > 0 or count == 0
    full = pc.model(chunk[2], chunk[1], chunk[3], qid, rec, ops)
    assert int(full[3][:, 26].sum()) > 0  # the fixture has deletions
    # the Python wrapper returns the same arrays
    got = path_pileup_host(chunk[2], chunk[1], chunk[3], qid, rec, ops, profile=True)
    pc.assert_same(got, full, "wrapper")
    assert len(path_pileup_host(chunk[2], chunk[1], chunk[3], qid, rec, ops)) == 3


def test_host_hand_made_and_edge_paths(data_root):
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    call = pc.host_call(native.load(), chunk)
    qid, rec, ops = pr.hand_paths(nq, L, len(dbseq))
    want = pc.check_against_model(call, chunk, qid, rec, ops, "hand")
    # an empty path and an insertion-only path add nothing; the D-only run does
    assert int(want[0].sum()) == sum(c for c in pr.HAND_COLUMNS) - 5 - 36 - 6 - 1 - 127
    for name, (q, r, o) in pc.edge_cases(nq, L, len(dbseq)).items():
        w = pc.check_against_model(call, chunk, q, r, o, name)
        if name == "copies_300":
            assert w[0][70:90].tolist() == [300] * 20 and int(w[0].sum()) == 6000
        if name == "d_across_edge":
            assert w[3][60:70, 26].tolist() == [1] * 10 and w[2][60:70].tolist() == [255] * 10
        if name == "i_at_edge":
            assert w[0][54:74].tolist() == [1] * 20 and int(w[0].sum()) == 20


def test_consensus_rules():
    """The lowest slot wins a tie; codes from 25 up and deletions give 255 with depth > 0."""
    prof = np.zeros((5, 32), dtype=np.uint32)
    prof[0, [3, 7]] = 2          # a tie: slot 3
    prof[1, 25] = 4              # only a code >= 25
    prof[2, 26] = 1              # only a deletion
    prof[3, [24, 26]] = [1, 9]   # '*' once, nine deletions
    depth, ident, cons = pc.finish(prof, np.array([7, 25, 3, 24, 0], dtype=np.uint8))
    assert cons.tolist() == [3, 255, 255, 24, 255] and depth.tolist() == [4, 4, 1, 10, 0]
    assert ident.tolist() == [2, 4, 0, 1, 0]
    assert consensus_text(cons, depth) == b"D--*."


def test_struct_layout():
    assert ctypes.sizeof(native.GhostmSubjectPileup) == SUBJECT_PILEUP_DTYPE.itemsize == 40
    for name, _ in native.GhostmSubjectPileup._fields_:
        f = getattr(native.GhostmSubjectPileup, name)
        assert SUBJECT_PILEUP_DTYPE.fields[name][1] == f.offset, name
        assert SUBJECT_PILEUP_DTYPE.fields[name][0].itemsize == f.size, name
    assert [n for n, _ in native.GhostmSubjectPileup._fields_] == list(SUBJECT_PILEUP_DTYPE.names)
    stats = [n for n, _ in native.GhostmStats._fields_]
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]


def test_host_refusals(data_root):
    d, chunk = pr.build_tiny(data_root)
    nq, L, qseq, dbseq, pos = chunk
    pc.check_refusals(pc.host_call(native.load(), chunk), nq, L, len(dbseq), gpu=False)
