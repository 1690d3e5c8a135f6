"""Replacing a session's database, the parts that need no GPU: db's chunk-cut
rule as a host function (GhostmDbChunkCuts, db_set.h) against the files
`ghostm db -l 1` writes, its refusals, the C ABI's refusals on null arguments
and `ghostm search`'s usage errors around -f and -d (exit 1 before any device
call)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import cases
from ghostm_amd import GhostmError, db_chunk_cuts, native

MB = 1 << 20


def db_nseq(prefix):
    division = int(np.fromfile(prefix + ".inf", dtype="<i4", count=1)[0])
    return [int(np.fromfile(f"{prefix}_{c}.inf", dtype="<u4", count=1)[0]) for c in range(division)]


def write_lengths(path, lens):
    """A FASTA file of records of these lengths (one letter repeated: only the
    lengths matter to the cut)."""
    with open(path, "w") as f:
        for i, n in enumerate(lens):
            f.write(f">s{i}\n" + ("A" * n + "\n" if n else ""))


def test_chunk_cuts_equal_db_files(tmp_path, built):
    """Random lengths over several 1 MiB chunks, with one record that fills a
    chunk exactly (length + 1 = 1 MiB) and the same record a byte over what is
    left of its chunk, after an empty record (so it is carried)."""
    r = random.Random(21)
    lens = [r.randint(0, 60000) for _ in range(60)]
    lens += [MB - 1]             # alone it fills a chunk exactly ...
    lens += [0, MB - 1]          # ... and after an empty record (1 byte) it is a byte over: carried
    lens += [r.randint(0, 60000) for _ in range(40)]
    write_lengths(tmp_path / "db.fa", lens)
    subprocess.run([cases.GHOSTM, "db", "-i", str(tmp_path / "db.fa"), "-o", str(tmp_path / "db"), "-l", "1"],
                   check=True, capture_output=True)
    nseq = db_nseq(str(tmp_path / "db"))
    assert len(nseq) >= 5
    cuts = db_chunk_cuts(lens, chunk_mb=1)
    assert [int(x) for x in np.diff(cuts.astype(np.int64))] == nseq
    # the exact fill is a chunk of its own or closes one; the carried record starts the next
    at = 60
    sums = [sum(n + 1 for n in lens[int(a):int(b)]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert max(sums) <= MB
    assert at + 2 in [int(c) for c in cuts], "the record a byte over the rest of its chunk starts a chunk"


def test_chunk_cuts_edges(built):
    # length + 1 is what counts: MB - 1 letters fill 1 MiB, one more record is carried
    assert list(db_chunk_cuts([MB - 1, 0, MB - 2, 0], chunk_mb=1)) == [0, 1, 3, 4]
    assert list(db_chunk_cuts([MB - 2, 0, 0], chunk_mb=1)) == [0, 2, 3]
    assert list(db_chunk_cuts([], chunk_mb=1)) == [0]
    assert list(db_chunk_cuts([5, 7, 0])) == [0, 3]  # the default: 128 MiB


@pytest.mark.parametrize("lens", [[MB, 5], [5, MB], [5, MB, 5]], ids=["first", "later", "middle"])
def test_chunk_cuts_refuse_a_record_over_the_limit(built, lens):
    """-1 in either position (where `ghostm db` writes an empty database for the
    first record and "too small max length" for a later one)."""
    with pytest.raises(GhostmError, match="too small max length"):
        db_chunk_cuts(lens, chunk_mb=1)
    lib = native.load()
    arr = np.array(lens, dtype=np.uint32)
    assert lib.GhostmDbChunkCuts(arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(arr), 1, None, 0) == -1


def test_db_itself_on_a_record_over_the_limit(tmp_path, built):
    """The formatter's two behaviours the header comment describes."""
    write_lengths(tmp_path / "a.fa", [MB, 5])
    r = subprocess.run([cases.GHOSTM, "db", "-i", str(tmp_path / "a.fa"), "-o", str(tmp_path / "a"), "-l", "1"],
                       capture_output=True)
    assert db_nseq(str(tmp_path / "a")) == [] and b"too small" not in r.stderr
    write_lengths(tmp_path / "b.fa", [5, MB])
    r = subprocess.run([cases.GHOSTM, "db", "-i", str(tmp_path / "b.fa"), "-o", str(tmp_path / "b"), "-l", "1"],
                       capture_output=True)
    assert b"too small max length" in r.stderr


def test_chunk_cuts_reject_2048_mb(built):
    with pytest.raises(GhostmError, match="2047"):
        db_chunk_cuts([5, 7], chunk_mb=2048)
    assert list(db_chunk_cuts([5, 7], chunk_mb=2047)) == [0, 2]


def test_null_session_and_arguments_are_errors(built):
    lib = native.load()
    calls = [
        lambda: lib.GhostmSessionSetDbFasta(None, b"x.fa", 4, 0),
        lambda: lib.GhostmSessionSetDb(None, None, 0, None, None, None, 0, 0, 4, 0),
        lambda: lib.GhostmSessionDbIndex(None, 0, None, 0, None, 0),
    ]
    for call in calls:
        assert call() != 0
        assert native.last_error()
    assert lib.GhostmSessionDbRecords(None, 0, None, 0) == ctypes.c_size_t(-1).value
    assert native.last_error()
    assert lib.GhostmSessionDbChunks(None, None, 0) == 0
    # -d does not go with a session without a database (refused before the device is touched)
    args = ["aln", "-d", "nowhere"]
    assert not lib.GhostmSessionCreateQueries(len(args), native.argv_array(args))
    assert "without a database" in native.last_error()


def test_db_set_stats_are_a_struct_of_their_own(built):
    """GhostmDbSetStats (GhostmSessionDbStats) holds the six counters; GhostmStats
    keeps the size the library reports and holds none of them."""
    lib = native.load()
    assert [n for n, _ in native.GhostmDbSetStats._fields_] == [
        "seconds_db_format", "seconds_db_code", "db_format_launches", "db_sets", "seconds_db_read", "seconds_db_load"]
    assert ctypes.sizeof(native.GhostmDbSetStats) == 48
    st = native.GhostmStats()
    assert lib.GhostmStageStats(ctypes.byref(st), ctypes.sizeof(st)) == ctypes.sizeof(st)
    assert not [n for n, _ in native.GhostmStats._fields_ if "_db_" in n or n.startswith("db_")]
    db = native.GhostmDbSetStats()
    assert lib.GhostmSessionDbStats(None, ctypes.byref(db), ctypes.sizeof(db)) == 0
    assert lib.GhostmSessionDbStats(None, None, 0) == 0


@pytest.mark.parametrize("args", [
    ["-f", "db.fa", "-d", "db", "a.fa", "a.out"],   # both
    ["a.fa", "a.out"],                              # neither
    ["-k", "4", "a.fa", "a.out"],
    ["-f", "db.fa"],                                # no pairs
    ["-f", "db.fa", "a.fa"],
])
def test_search_usage_errors_exit_1(tmp_path, built, args):
    r = subprocess.run([cases.GHOSTM, "search"] + args, cwd=tmp_path, capture_output=True)
    assert r.returncode == 1
    assert b"search:" in r.stderr
    assert os.listdir(tmp_path) == []
