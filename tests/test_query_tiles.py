"""The tile plan of a tiled query set, the parts that need no GPU
(GhostmQueryTilePlan, ghostm_amd.tile_plan): the plan's guarantees over every
small source length, width and step, the max_len cut, the per-record limit, the
tile-major order of a DNA read, and the refusals of the C ABI and the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cases
from ghostm_amd import GhostmError, native, tile_plan

WIDTHS = [1, 2, 63, 64, 65, 127]


def starts_by_record(tiles, n):
    """[starts] per source record of a protein plan, in output order."""
    out = [[] for _ in range(n)]
    for rec, off in zip(tiles["record"].tolist(), tiles["offset"].tolist()):
        out[rec].append(off)
    return out


@pytest.mark.parametrize("W", WIDTHS)
def test_plan_guarantees(built, W):
    """All m <= 4 W + 3 and every step 1..W: strictly increasing starts, every
    letter covered, consecutive tiles overlapping by at least W - step, and
    every window of at most W - step + 1 letters wholly inside some tile."""
    lengths = np.arange(0, 4 * W + 4, dtype=np.uint32)
    for step in range(1, W + 1):
        tiles, cut = tile_plan(lengths, width=W, step=step)
        assert cut == 0
        assert (tiles["frame"] == 0).all()
        assert (tiles["letters"] == lengths[tiles["record"]]).all()
        for m, starts in enumerate(starts_by_record(tiles, len(lengths))):
            want = 1 if m <= W else 1 + -(-(m - W) // step)
            assert len(starts) == want, (W, step, m)
            s = np.array(starts, dtype=np.int64)
            assert s[0] == 0
            if m <= W:
                continue
            assert (np.diff(s) > 0).all(), (W, step, m)
            assert s[-1] == m - W and (s[:-1] == np.arange(len(s) - 1) * step).all()
            # coverage: the tiles' union is [0, m) and neighbours overlap by at least W - step
            assert (s[1:] <= s[:-1] + W).all() and s[-1] + W == m
            assert (s[:-1] + W - s[1:] >= W - step).all(), (W, step, m)
            # every window [a, a + W - step + 1) inside [0, m) lies in the last tile starting at or before a
            win = W - step + 1
            a = np.arange(0, m - win + 1)
            owner = s[np.searchsorted(s, a, side="right") - 1]
            assert (a + win <= owner + W).all(), (W, step, m)


def test_max_len_cuts_first(built):
    tiles, cut = tile_plan([10, 20, 21, 300], width=8, step=4, max_len=20)
    assert cut == 2
    assert tiles["letters"][tiles["record"] == 1][0] == 20
    assert tiles["letters"][tiles["record"] == 2][0] == 20
    assert tiles["letters"][tiles["record"] == 3][0] == 20
    assert tiles["offset"][tiles["record"] == 3].tolist() == [0, 4, 8, 12]
    # DNA: max_len in nt, six records counted per read cut
    tiles, cut = tile_plan([100, 61], width=30, dna=True, step=5, max_len=60)
    assert cut == 12 and (tiles["letters"] == 20).all()
    assert tile_plan([100], width=30, dna=True, step=5)[1] == 0


def test_dna_is_tile_major_frame_minor(built):
    # width 30 nt -> W = 10 letters; a read of 77 nt has 25 letters per frame: tiles at 0, 6, 12, 15
    tiles, _ = tile_plan([12, 77], width=30, dna=True, step=6)
    first = tiles[tiles["record"] == 0]
    assert first["offset"].tolist() == [0] * 6 and first["frame"].tolist() == list(range(6))  # today's six records
    assert (first["letters"] == 4).all()
    second = tiles[tiles["record"] == 1]
    assert second["frame"].tolist() == list(range(6)) * 4
    assert second["offset"].tolist() == [0] * 6 + [6] * 6 + [12] * 6 + [15] * 6
    assert (second["letters"] == 25).all()
    assert (tiles["record"] == [0] * 6 + [1] * 24).all()


def test_per_record_limit(built):
    """At most 1024 output records per source record: 1024 protein tiles, 170
    tiles x 6 frames."""
    W = 127
    assert len(tile_plan([W + 1023], width=W, step=1)[0]) == 1024
    with pytest.raises(GhostmError, match="limit"):
        tile_plan([W + 1024], width=W, step=1)
    assert len(tile_plan([3 * (W + 169)], width=3 * W, dna=True, step=1)[0]) == 170 * 6
    with pytest.raises(GhostmError, match="limit"):
        tile_plan([3 * (W + 170)], width=3 * W, dna=True, step=1)
    assert len(tile_plan([64 * W], width=W, step=W)[0]) == 64  # at least 64 tiles x 6 frames pass
    assert len(tile_plan([3 * 64 * W], width=3 * W, dna=True, step=W)[0]) == 64 * 6


def test_width_rule_is_the_setters(built):
    # over 127 the width is capped; a DNA set's is a third of the read length given
    assert tile_plan([300], width=500, step=127)[0]["offset"].tolist() == [0, 127, 173]
    assert tile_plan([75], width=75, dna=True, step=25)[0]["letters"].tolist() == [25] * 6


def test_refusals(built):
    lib = native.load()
    for step in (0, 9):
        with pytest.raises(GhostmError, match="step"):
            tile_plan([5], width=8, step=step)
    with pytest.raises(GhostmError, match="step"):
        tile_plan([5], width=2, dna=True, step=1)  # a DNA width under one codon: W = 0
    assert lib.GhostmQueryTilePlan(None, 3, 8, 0, 0, 4, None, 0, None) == -1
    assert "null" in native.last_error()
    cut = ctypes.c_uint64(0)
    calls = [
        lambda: lib.GhostmSessionSetQueriesTiled(None, None, 0, None, None, None, 0, 0, 75, 0, 0, 0, 1),
        lambda: lib.GhostmSessionSetQueriesFastaTiled(None, b"x.fa", 75, 0, 0, 0, 1, ctypes.byref(cut)),
    ]
    for call in calls:
        assert call() != 0
        assert native.last_error()
    assert lib.GhostmSessionQueryTiles(None, None, 0) == 0
    assert ctypes.sizeof(native.GhostmQueryTile) == 16


def test_search_usage_minus_x_needs_minus_t(tmp_path, built):
    r = subprocess.run([cases.GHOSTM, "search", "-d", "db", "-X", "300", "a.fa", "a.out"], cwd=tmp_path,
                       capture_output=True)
    assert r.returncode == 1
    assert os.listdir(tmp_path) == []
