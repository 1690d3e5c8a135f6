"""Replacing a session's query set, the parts that need no GPU: the refusals of
the C ABI on null arguments, `ghostm search`'s usage errors (exit 1 before any
device call, no output file) and qry's chunk-cut rule as a host function
(GhostmQueryChunkCuts) against the files `ghostm qry` writes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cases
from ghostm_amd import GhostmError, native, query_chunk_cuts


def test_null_session_and_arguments_are_errors(built):
    lib = native.load()
    cut = ctypes.c_uint64(0)
    calls = [
        lambda: lib.GhostmSessionSetQueriesFasta(None, b"x.fa", 75, 0, 0, ctypes.byref(cut)),
        lambda: lib.GhostmSessionSetQueries(None, None, 0, None, None, None, 0, 0, 75, 0, 0),
        lambda: lib.GhostmSessionSetOutputFile(None, b"x.out"),
    ]
    for call in calls:
        assert call() != 0
        assert native.last_error()
    assert lib.GhostmSessionQueryRecords(None, 0, None, 0) == ctypes.c_size_t(-1).value
    assert native.last_error()
    assert lib.GhostmSessionQueryLengths(None, None, 0) == 0
    # -i, -S or -L do not go with a database session (refused before the device is touched)
    for extra in (["-i", "x"], ["-S", "0"], ["-L", "1"]):
        args = ["aln", "-d", "nowhere"] + extra
        assert not lib.GhostmSessionCreateDb(len(args), native.argv_array(args))
        assert "database session" in native.last_error()


@pytest.mark.parametrize("args", [
    [],                                    # no pairs
    ["a.fa"],                              # odd positional count
    ["a.fa", "a.out", "b.fa"],
    ["-i", "x", "a.fa", "a.out"],
    ["-o", "x", "a.fa", "a.out"],
    ["-S", "0", "a.fa", "a.out"],
    ["-L", "0", "a.fa", "a.out"],
])
def test_search_usage_errors_exit_1(tmp_path, built, args):
    r = subprocess.run([cases.GHOSTM, "search", "-d", "db"] + args, cwd=tmp_path, capture_output=True)
    assert r.returncode == 1
    assert b"search:" in r.stderr
    assert os.listdir(tmp_path) == []


def fasta_lengths(path):
    lens, n = [], None
    for line in open(path):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            if n is not None:
                lens.append(n)
            n = 0
        elif n is not None:
            n += len(line)
    if n is not None:
        lens.append(n)
    return lens


def qry_nseq(prefix):
    division = int(np.fromfile(prefix + ".inf", dtype="<i4", count=1)[0])
    return [int(np.fromfile(f"{prefix}_{c}.inf", dtype="<u4", count=1)[0]) for c in range(division)]


def test_chunk_cuts_equal_qry_files(dataset):
    d = dataset("syn_chunks")
    cuts = query_chunk_cuts(fasta_lengths(os.path.join(d, "q.fa")), chunk_mb=1)
    nseq = qry_nseq(os.path.join(d, "q"))
    assert len(nseq) == 2
    assert list(np.diff(cuts.astype(np.int64))) == nseq
    d = dataset("syn_dna")  # qry -t d with the default limit: six records per read
    cuts = query_chunk_cuts(fasta_lengths(os.path.join(d, "q.fa")), dna=True)
    assert [6 * int(x) for x in np.diff(cuts.astype(np.int64))] == qry_nseq(os.path.join(d, "q"))


def test_chunk_cuts_dna_halved_limit(tmp_path, built):
    """-t d halves the limit: 3000 reads of 300 bases cut at 512 Ki letters, each
    read six records."""
    import random

    r = random.Random(3)
    fa = tmp_path / "d.fa"
    with open(fa, "w") as f:
        for i in range(3000):
            f.write(f">r{i}\n" + "".join(r.choice("ACGT") for _ in range(300 + (i % 7))) + "\n")
    subprocess.run([cases.GHOSTM, "qry", "-i", str(fa), "-o", str(tmp_path / "q"), "-t", "d", "-l", "300",
                    "-L", "1"], check=True, capture_output=True)
    nseq = qry_nseq(str(tmp_path / "q"))
    assert len(nseq) >= 2
    cuts = query_chunk_cuts(fasta_lengths(fa), chunk_mb=1, dna=True)
    assert [6 * int(x) for x in np.diff(cuts.astype(np.int64))] == nseq


def test_chunk_cuts_edges(built):
    mb = 1 << 20
    # a record that fills the limit exactly stays; the next is carried
    assert list(query_chunk_cuts([mb, 1, mb - 1, 1], chunk_mb=1)) == [0, 1, 3, 4]
    assert list(query_chunk_cuts([], chunk_mb=1)) == [0]
    # the first record of the file over the limit: qry writes no chunk at all
    assert list(query_chunk_cuts([mb + 1, 5], chunk_mb=1)) == [0]
    # a carried record over the limit: qry's "too small max length"
    with pytest.raises(GhostmError):
        query_chunk_cuts([5, mb + 1], chunk_mb=1)
