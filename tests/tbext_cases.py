"""Shared by tests/test_traceback_ext_host.py and tests/test_gpu_traceback_ext.py
(not a test module): the indel fixture, a Python model of the extended
traceback written from its contract, and the chunk-file helpers.

The contract (include/ghostm_hip.h, TraceBackExtGpu): the reference's reverse
DP (aligner.cpp:771-949), columns j = 0.. walking the DB backwards from db_end,
rows k = L-1..0, every H cell carrying (len, match, mism, gapopen, origin, op)
taken from the H cell it steps from, also for the E and F chains."""
from __future__ import annotations

import ctypes
import functools
import os
import random
import subprocess
import zlib

import numpy as np

import cases

AA = "ARNDCQEGHILKMFPSTWYV"
END = 25
NONE, DIAG, INS, DEL = 0, 1, 2, 3


def blosum62():
    return cases.parse_ncbi_matrix(os.path.join(cases.GOLDEN, "matrices", "BLOSUM62"))


def pam250():
    return cases.parse_ncbi_matrix(cases.PAM250)


def codes(s: str) -> np.ndarray:
    return np.array([AA.index(c) for c in s], dtype=np.uint8)


# ---------------------------------------------------------------- Python model
def py_model(qs, db, M, end, base, open_gap=-11, extend_gap=-1, max_cols=None):
    """One hit. Returns dict(start, len, match, q_start, q_end, mism, gapopen,
    dels): the tuple of the first cell, in the reference's loop order, that
    reaches the strict maximum (dels = its F steps, for the invariants).
    max_cols stops the DP after that many columns (the first maximal column is
    the same when it is at least the hit's end - start + 1)."""
    L = len(qs)
    qs = [int(x) for x in qs]
    M = [int(x) for x in M]
    zero = (0, 0, 0, 0, 0, NONE, 0)  # len, match, mism, gapopen, origin, op, dels
    H = [0] * (L + 1)
    E = [0] * (L + 1)
    T = [zero] * (L + 1)
    width = end + 1 if end < base else base
    if max_cols is not None:
        width = min(width, max_cols)
    best, best_j, best_k, best_t = 0, 0, 0, zero
    for j in range(width):
        c = int(db[end - j])
        if c == END:
            break
        row = M[c * 32:(c + 1) * 32]
        diag, F, dt = 0, 0, zero
        for k in range(L - 1, -1, -1):
            cell, t = 0, zero
            s = diag + row[qs[k]]
            if s > 0:
                eq = 1 if c == qs[k] else 0
                cell = s
                t = (dt[0] + 1, dt[1] + eq, dt[2] + 1 - eq, dt[3], k if dt[0] == 0 else dt[4], DIAG, dt[6])
            E[k] = max(E[k] + extend_gap, H[k] + open_gap)
            if E[k] > cell:
                p = T[k]
                cell = E[k]
                t = (p[0] + 1, p[1], p[2], p[3] + (1 if p[5] != INS else 0), k if p[0] == 0 else p[4], INS, p[6])
            F = max(F + extend_gap, H[k + 1] + open_gap)
            if F > cell:
                p = T[k + 1]
                cell = F
                t = (p[0] + 1, p[1], p[2], p[3] + (1 if p[5] != DEL else 0), k if p[0] == 0 else p[4], DEL, p[6] + 1)
            diag, H[k] = H[k], cell
            dt, T[k] = T[k], t
            if cell > best:
                best, best_j, best_k, best_t = cell, j, k, t
    return dict(start=end - best_j, len=best_t[0], match=best_t[1], q_start=best_k, q_end=best_t[4],
                mism=best_t[2], gapopen=best_t[3], dels=best_t[6])


def check_invariants(alen, match, ext, dels=None):
    """The four invariants of the contract on arrays of hits (dels: the F steps
    where a model reports them; otherwise only their range is checked)."""
    alen = np.asarray(alen, dtype=np.int64)
    match = np.asarray(match, dtype=np.int64)
    mism = ext["mismatches"].astype(np.int64)
    opens = ext["gap_opens"].astype(np.int64)
    gaps = alen - match - mism
    assert (gaps >= 0).all()                                  # aln_len = match + mismatches + gaps
    span = ext["q_end"].astype(np.int64) - ext["q_start"].astype(np.int64) + 1
    subj_gaps = span - match - mism
    live = alen > 0
    assert ((subj_gaps >= 0) & (subj_gaps <= gaps))[live].all()  # query span = match + mism + subject gaps
    if dels is not None:
        assert np.array_equal(subj_gaps[live], np.asarray(dels, dtype=np.int64)[live])
    assert np.array_equal(opens == 0, gaps == 0)
    assert (opens <= gaps).all()
    return gaps


# ---------------------------------------------------------------- the fixture
def _fasta(name, seq):
    return f">{name}\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60))


def write_fixture(d: str, L: int) -> None:
    """30 subjects of 150-300 uniform residues; 60 reads of L + 4 residues of
    subject i % 30 with planted indels by i % 4 (none; 1-3 deleted in the middle
    third; 1-3 inserted there; two deleted at L/4 and one inserted at 2L/3), then
    three substitutions, cut to L. Reads 0-3 start at offset 0 of subjects 0-3:
    one reverse window is clipped at DB position 0, three end at a subject END."""
    random.seed(3)
    subjects = ["".join(random.choice(AA) for _ in range(random.randint(150, 300))) for _ in range(30)]
    reads = []
    for i in range(60):
        s = subjects[i % 30]
        off = 0 if i < 4 else random.randint(0, len(s) - (L + 4))
        r = list(s[off:off + L + 4])
        kind = i % 4
        if kind == 1:
            p, n = random.randint(L // 3, 2 * L // 3), random.randint(1, 3)
            del r[p:p + n]
        elif kind == 2:
            p, n = random.randint(L // 3, 2 * L // 3), random.randint(1, 3)
            r[p:p] = [random.choice(AA) for _ in range(n)]
        elif kind == 3:
            del r[L // 4:L // 4 + 2]
            r[2 * L // 3:2 * L // 3] = [random.choice(AA)]
        for _ in range(3):
            r[random.randrange(len(r))] = random.choice(AA)
        reads.append("".join(r[:L]))
    with open(os.path.join(d, "db.fa"), "w") as f:
        f.write("".join(_fasta(f"s{i}", s) for i, s in enumerate(subjects)))
    with open(os.path.join(d, "q.fa"), "w") as f:
        f.write("".join(_fasta(f"r{i}", s) for i, s in enumerate(reads)))


def build_fixture(root: str, L: int) -> str:
    d = os.path.join(root, f"tbext_L{L}")
    stamp = os.path.join(d, ".done")
    if not os.path.exists(stamp):
        os.makedirs(d, exist_ok=True)
        write_fixture(d, L)
        subprocess.run([cases.GHOSTM, "db", "-i", f"{d}/db.fa", "-o", f"{d}/db"], check=True, capture_output=True)
        subprocess.run([cases.GHOSTM, "qry", "-i", f"{d}/q.fa", "-o", f"{d}/q", "-l", str(L)], check=True,
                       capture_output=True)
        open(stamp, "w").close()
    return d


def load_chunk(d, qi=0, di=0, qprefix="q", dprefix="db"):
    """(nq, L, qseq[nq*L], dbseq, pos) of query chunk qi and DB chunk di."""
    inf = np.fromfile(f"{d}/{qprefix}_{qi}.inf", dtype="<u4")
    nq, L = int(inf[0]), int(inf[1])
    qseq = np.fromfile(f"{d}/{qprefix}_{qi}.seq", dtype=np.uint8)[: nq * L]
    dinf = np.fromfile(f"{d}/{dprefix}_{di}.inf", dtype="<u4")
    dbseq = np.fromfile(f"{d}/{dprefix}_{di}.seq", dtype=np.uint8)[: int(dinf[1])]
    pos = np.fromfile(f"{d}/{dprefix}_{di}.pos", dtype="<u4")[: int(dinf[0])]
    return nq, L, np.ascontiguousarray(qseq), np.ascontiguousarray(dbseq), pos


def load_index(d, di=0, dprefix="db"):
    raw = np.fromfile(f"{d}/{dprefix}_{di}.ind", dtype="<u4")
    seed, kcl, npos = (int(x) for x in raw[:3])
    return seed, np.ascontiguousarray(raw[3:3 + kcl]), np.ascontiguousarray(raw[3 + kcl:3 + kcl + npos])


def oracle_tb(d, opts, dump_dir, n=60):
    """The first n records {qid, end, start, aln_len, aln_match} of the oracle's
    traceback dump for `aln opts` on dataset d."""
    os.makedirs(dump_dir, exist_ok=True)
    prefix = os.path.join(dump_dir, "dump")
    for suffix in (".tb", ".cand"):
        if os.path.exists(prefix + suffix):
            os.remove(prefix + suffix)
    cases.run_aln(cases.ORACLE, d, ["-y", "1"] + list(opts), {"GHOSTM_ORACLE_DUMP": prefix},
                  os.path.join(dump_dir, "o"))
    tb = np.fromfile(prefix + ".tb", dtype="<u4").reshape(-1, 5)
    assert len(tb) >= n, f"the oracle traced {len(tb)} hits, fewer than {n}"
    return np.ascontiguousarray(tb[:n])


def assert_gapped(alen, match, ext):
    """A set without gaps cannot pass silently: at least 20 gapped hits and at
    least 5 with two or more opens (the reference alone gives 45 and 16-20)."""
    gaps = alen.astype(np.int64) - match.astype(np.int64) - ext["mismatches"].astype(np.int64)
    assert int((gaps > 0).sum()) >= 20, int((gaps > 0).sum())
    assert int((ext["gap_opens"] >= 2).sum()) >= 5, int((ext["gap_opens"] >= 2).sum())


@functools.lru_cache(maxsize=None)
def fixture_hits(root: str, L: int, opts: tuple = ()):
    """The fixture at L with the oracle's 60 hits for `opts`: (d, chunk, tb)."""
    d = build_fixture(root, L)
    tb = oracle_tb(d, list(opts), os.path.join(d, "dump_%08x" % zlib.crc32(" ".join(opts).encode())))
    return d, load_chunk(d), tb


# ---------------------------------------------------------------- stage level
def _p(a, t=ctypes.c_uint32):
    return a.ctypes.data_as(ctypes.POINTER(t))


def stage_check(lib, d, chunk, tb, M, base, open_gap=-11, extend_gap=-1):
    """InitGpu/SetOptionGpu/SetQueryGpu/SetDbGpu, then TraceBackExtGpu on the hits
    of tb (with and without the known starts; 60, 1 and 0 hits): every output
    equals the host model's, (start, len, match) equal TraceBackGpu's. Returns
    the host model's (start, len, match, ext)."""
    from ghostm_amd import HIT_EXT_DTYPE, native, traceback_ext_host

    nq, L, qseq, dbseq, pos = chunk
    seed, kc, ipos = load_index(d)
    M = np.ascontiguousarray(M, dtype=np.int32)
    assert lib.InitGpu() == 0
    assert lib.SetOptionGpu(1 << 27, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0) == 0, native.last_error()
    assert lib.SetQueryGpu(_p(qseq, ctypes.c_uint8), nq, L) == 0, native.last_error()
    assert lib.SetDbGpu(_p(dbseq, ctypes.c_uint8), len(dbseq), _p(kc), len(kc), _p(ipos), len(ipos)) == 0
    qid = np.ascontiguousarray(tb[:, 0])
    end = np.ascontiguousarray(tb[:, 1])
    want = traceback_ext_host(qseq, L, dbseq, M, qid, end, base, open_gap, extend_gap)
    w_start, w_len, w_match, w_ext = want
    n = len(qid)
    # K3 as it is today
    k_start, k_len, k_match = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    k_id = np.zeros(n, dtype=np.float32)
    assert lib.TraceBackGpu(n, _p(qid), _p(end), L, base, open_gap, extend_gap, _p(k_start), _p(k_len), _p(k_match),
                            k_id.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 0, native.last_error()
    for count in (n, 1, 0):
        for starts_in in (None, np.ascontiguousarray(w_start[:count])):
            g_start, g_len, g_match = (np.full(count + 1, 0xDEAD, dtype=np.uint32) for _ in range(3))
            g_ext = np.zeros(count + 1, dtype=HIT_EXT_DTYPE)
            rc = lib.TraceBackExtGpu(count, _p(qid), _p(end), None if starts_in is None else _p(starts_in), L, base,
                                     open_gap, extend_gap, _p(g_start), _p(g_len), _p(g_match),
                                     g_ext.ctypes.data_as(ctypes.POINTER(native.GhostmHitExt)))
            assert rc == 0, native.last_error()
            assert g_start[count] == 0xDEAD and g_len[count] == 0xDEAD  # nothing written past the hits
            assert np.array_equal(g_start[:count], w_start[:count])
            assert np.array_equal(g_len[:count], w_len[:count])
            assert np.array_equal(g_match[:count], w_match[:count])
            assert np.array_equal(g_ext[:count], w_ext[:count])
            assert np.array_equal(g_start[:count], k_start[:count])
            assert np.array_equal(g_len[:count], k_len[:count])
            assert np.array_equal(g_match[:count], k_match[:count])
    assert lib.FreeGpu() == 0
    return want


# ---------------------------------------------------------------- session level
def dataset_chunks(d, qprefix="q", dprefix="db"):
    """(query chunks, DB chunks) of a formatted dataset: per query chunk (global
    base, nq, L, qseq, names), per DB chunk (global base, nseq, dbseq, pos)."""
    qs, dbs = [], []
    base = 0
    i = 0
    while os.path.exists(f"{d}/{qprefix}_{i}.inf"):
        nq, L, qseq, _, _ = load_chunk(d, i, 0, qprefix, dprefix)
        names = open(f"{d}/{qprefix}_{i}.nam").read().split("\n")[:nq]
        qs.append((base, nq, L, qseq, names))
        base += nq
        i += 1
    base = 0
    i = 0
    while os.path.exists(f"{d}/{dprefix}_{i}.inf"):
        _, _, _, dbseq, pos = load_chunk(d, 0, i, qprefix, dprefix)
        dbs.append((base, len(pos), dbseq, pos))
        base += len(pos)
        i += 1
    return qs, dbs


def session_expected(d, hits, M, base_of, open_gap=-11, extend_gap=-1):
    """The host model's GhostmHitExt of every session hit, from the formatted
    files: the hit's chunk-local query, absolute end and start. A hit record
    names the last query of its name group; the query that scored is the
    group's first one that reproduces the hit's (db_start, aln_len, aln_match).
    Returns (ext, inputs) with inputs[h] = (query chunk, local query, DB chunk,
    absolute end, absolute start)."""
    from ghostm_amd import HIT_EXT_DTYPE, traceback_ext_host

    qs, dbs = dataset_chunks(d)
    want = np.zeros(len(hits), dtype=HIT_EXT_DTYPE)
    inputs = [None] * len(hits)
    qc = np.searchsorted([q[0] for q in qs], hits["query_id"], side="right") - 1
    dc = np.searchsorted([x[0] for x in dbs], hits["db_id"], side="right") - 1
    for qi, (qbase, nq, L, qseq, names) in enumerate(qs):
        for di, (dbase, nsub, dbseq, pos) in enumerate(dbs):
            idx = np.nonzero((qc == qi) & (dc == di))[0]
            if len(idx) == 0:
                continue
            owner, qid, end = [], [], []
            for h in idx:
                last = int(hits["query_id"][h]) - qbase
                first = last
                while first > 0 and names[first - 1] == names[last]:
                    first -= 1
                p = int(pos[int(hits["db_id"][h]) - dbase])
                for f in range(first, last + 1):
                    owner.append(h)
                    qid.append(f)
                    end.append(p + int(hits["db_end"][h]))
            start, alen, match, ext = traceback_ext_host(qseq, L, dbseq, M, qid, end, base_of(L), open_gap, extend_gap)
            done = set()
            for k, h in enumerate(owner):
                p = int(pos[int(hits["db_id"][h]) - dbase])
                if h in done or (start[k], alen[k], match[k]) != (p + hits["db_start"][h], hits["aln_len"][h],
                                                                  hits["aln_match"][h]):
                    continue
                done.add(h)
                want[h] = ext[k]
                inputs[h] = (qi, qid[k], di, end[k], int(start[k]))
            assert len(done) == len(idx), "a hit's alignment is reproduced by no query of its name group"
    return want, inputs
