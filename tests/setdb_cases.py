"""Shared by tests/test_gpu_set_db.py and tests/setdb_poison_child.py (not a test
module itself): the FASTA files of the kernel-level edge set, the reader of the
files `ghostm db` writes, and the comparison of a session's resident database
with them. Every comparison is byte equality against the CPU formatter
(`ghostm db` without -D, pinned to the reference by tests/test_formatter.py)."""
import os
import random
import subprocess

import numpy as np

import cases

AA = "ARNDCQEGHILKMFPSTWYV"
VEC = 16      # bytes per lane of the coding kernel (kernels.h kDbCodeVec)
TILE = 4096   # bytes per workgroup (kDbCodeTile)

# chunk lengths in bytes, either side of the kernel's lane (16), wave (1024 is
# between 257 and 4095; 63..65 and 255..257 are the issue's), and workgroup
# (4096) widths
CHUNK_BYTES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


def write_fasta(path, recs):
    with open(path, "w") as f:
        for name, seq in recs:
            f.write(f">{name}\n" + (seq + "\n" if seq else ""))


def read_fasta(path):
    recs = []
    for line in open(path):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            recs.append([line[1:].lstrip("> "), ""])
        elif recs and line:
            recs[-1][1] += line
    return recs


def records_of_bytes(nbytes, r):
    """Records whose letters and ENDs make a chunk of exactly nbytes bytes, cut so
    that a record's END falls at the start (byte 0 of 16), inside (byte 7) and at
    the end (byte 15) of a vector group, in the first two and the last two
    groups; the chunk's last byte is the last record's END."""
    groups = sorted({g for g in (0, 1, (nbytes - 1) // VEC - 1, (nbytes - 1) // VEC) if g >= 0})
    ends = sorted({g * VEC + o for g in groups for o in (0, 7, 15) if g * VEC + o < nbytes - 1} | {nbytes - 1})
    recs, at = [], 0
    for i, e in enumerate(ends):
        recs.append((f"b{nbytes}_{i}", "".join(r.choice(AA) for _ in range(e - at))))
        at = e + 1
    assert sum(len(s) + 1 for _, s in recs) == nbytes
    return recs


def edge_records(k, r):
    """Subject lengths around the seed span (k contiguous positions), empty
    records first, last and twice in a row, every kind of letter, and an X at
    every place of a seed window."""
    rand = lambda n: "".join(r.choice(AA) for _ in range(n))  # noqa: E731
    recs = [("empty_first", "")]
    for n in (0, 1, k - 1, k, k + 1):
        recs.append((f"len{n}", rand(n)))
    recs += [("empty_a", ""), ("empty_b", ""),
             ("lower", rand(30).lower()), ("ambiguous", "MK" + "BZJX*" + rand(2 * k) + "bzjx*" + rand(k)),
             ("unknown", rand(k + 1) + "UO" + rand(k + 1) + "0123456789" + rand(k + 1) + "-uo" + rand(k + 1)),
             ("mixed_case", "".join(ch.lower() if i % 3 else ch for i, ch in enumerate(rand(40))))]
    for t in range(k):  # one X at place t of the window that starts at 10
        s = list(rand(10 + 2 * k + 10))
        s[10 + t] = "X"
        recs.append((f"x_at{t}", "".join(s)))
    recs += [("just_span_again", rand(k)), ("tail", rand(3 * k)), ("empty_last", "")]
    return recs


def db_files(prefix):
    """The chunks of the files `ghostm db` wrote: header values and arrays."""
    division = int(np.fromfile(prefix + ".inf", dtype="<i4", count=1)[0])
    out = []
    for c in range(division):
        nseq, length = (int(x) for x in np.fromfile(f"{prefix}_{c}.inf", dtype="<u4", count=2))
        ind = np.fromfile(f"{prefix}_{c}.ind", dtype="<u4")
        seed, kcl, npos = (int(x) for x in ind[:3])
        out.append(dict(id=c, nseq=nseq, len=length, seed=seed, kcl=kcl, npos=npos,
                        seq=np.fromfile(f"{prefix}_{c}.seq", dtype=np.uint8),
                        starts=np.fromfile(f"{prefix}_{c}.pos", dtype="<u4"),
                        kc=ind[3:3 + kcl], pos=ind[3 + kcl:3 + kcl + npos]))
        assert out[-1]["seq"].size == length and out[-1]["starts"].size == nseq
    return out


def format_db(fa, prefix, k=4, chunk_mb=0):
    opts = ["-k", str(k)] + (["-l", str(chunk_mb)] if chunk_mb else [])
    subprocess.run([cases.GHOSTM, "db", "-i", str(fa), "-o", str(prefix)] + opts, check=True, capture_output=True)
    return db_files(str(prefix))


def assert_resident_equals_files(s, want):
    """The session's database against the chunks of db_files(): db_chunks,
    db_records, db_index, and the subject starts (from the subject lengths a
    pile-up of a run reports: start[i + 1] = start[i] + length[i] + 1)."""
    info = s.db_chunks()
    assert info == [{f: w[f] for f in ("id", "nseq", "len", "seed", "kcl", "npos")} for w in want]
    for c, w in enumerate(want):
        got = s.db_records(c)
        assert got.size == w["len"] and got.tobytes() == w["seq"].tobytes(), f"chunk {c}: residues"
        seed, kc, pos = s.db_index(c)
        assert seed == w["seed"], f"chunk {c}: seed"
        assert kc.tobytes() == w["kc"].tobytes(), f"chunk {c}: keys_count"
        assert pos.tobytes() == w["pos"].tobytes(), f"chunk {c}: positions"
    s.run()
    lengths = s.pileup()[0]["length"].astype(np.int64)
    at = 0
    for c, w in enumerate(want):
        mine = lengths[at:at + w["nseq"]]
        starts = np.concatenate([[0], np.cumsum(mine + 1)[:-1]]) if w["nseq"] else np.zeros(0, dtype=np.int64)
        assert starts.tolist() == w["starts"].tolist(), f"chunk {c}: subject starts"
        at += w["nseq"]
    assert at == lengths.size


def check_fasta(s, fa, prefix, k=4, chunk_mb=0):
    want = format_db(fa, prefix, k, chunk_mb)
    s.set_db_fasta(str(fa), k=k, chunk_mb=chunk_mb)
    assert_resident_equals_files(s, want)
    return want


def kernel_edge_set(s, tmp, ks=(3, 4, 5)):
    """The whole kernel-level edge set on session s (files under tmp); returns
    the number of databases compared."""
    n = 0
    for nbytes in CHUNK_BYTES:
        k = ks[n % len(ks)]
        fa = os.path.join(tmp, f"b{nbytes}.fa")
        write_fasta(fa, records_of_bytes(nbytes, random.Random(nbytes)))
        want = check_fasta(s, fa, os.path.join(tmp, f"b{nbytes}"), k=k)
        assert [w["len"] for w in want] == [nbytes]
        n += 1
    for k in ks:
        fa = os.path.join(tmp, f"edges{k}.fa")
        write_fasta(fa, edge_records(k, random.Random(100 + k)))
        check_fasta(s, fa, os.path.join(tmp, f"edges{k}"), k=k)
        n += 1
    return n
