"""Shared by tests/test_traceback_path_host.py and tests/test_gpu_traceback_path.py
(not a test module): a Python model of the alignment path written from its
contract, the invariant checker that re-walks a path along the two sequences,
and the stage- and session-level comparisons with the host model.

The contract (include/ghostm_hip.h, TraceBackPathGpu): the extended
traceback's reverse DP (columns j = 0.. walking the DB backwards from db_end,
rows k = L-1..0, the same window and END break); every cell records
    hsel  the term H took: 0 zero, 1 diagonal, 2 E, 3 F (h = s if s > 0 else
          0, then E if E > h, then F if F > h, each strict)
    eext  1 only when E(j-1,k) + ext > H(j-1,k) + open (a tie opens)
    fext  the same for F
and the path is walked from the first strict maximum, in state H, towards
column 0 and row L-1:
    H, hsel 1   emit '=' (equal codes) or 'X', go to H(j-1, k+1)
    H, hsel 2/3 enter E / F at the same cell
    H, hsel 0   stop (also outside the computed columns or past row L-1)
    E           emit 'D', go to E(j-1, k) if eext else H(j-1, k)
    F           emit 'I', go to F(j, k+1) if fext else H(j, k+1)"""
from __future__ import annotations

import ctypes
import itertools
import os
import random
import re
import subprocess

import numpy as np

import tbext_cases as tx

OPS = "=XID"


# ---------------------------------------------------------------- Python model
def path_model(qs, db, M, end, base, open_gap=-11, extend_gap=-1, max_cols=None):
    """One hit: dict(score, q_start, q_end, s_start, s_end, ops) with ops the
    operation string, one character per residue pair or gap residue."""
    L = len(qs)
    qs = [int(x) for x in qs]
    M = [int(x) for x in M]
    width = end + 1 if end < base else base
    if max_cols is not None:
        width = min(width, max_cols)
    H = [0] * (L + 1)
    E = [0] * (L + 1)
    dirs = []  # per computed column: (hsel, eext, fext) of every row
    best, bj, bk = 0, 0, 0
    for j in range(width):
        c = int(db[end - j])
        if c == tx.END:
            break
        row = M[c * 32:(c + 1) * 32]
        diag, F = 0, 0
        col = [None] * L
        for k in range(L - 1, -1, -1):
            cell, sel = 0, 0
            s = diag + row[qs[k]]
            if s > 0:
                cell, sel = s, 1
            ee, eo = E[k] + extend_gap, H[k] + open_gap
            E[k] = max(ee, eo)
            if E[k] > cell:
                cell, sel = E[k], 2
            fe, fo = F + extend_gap, H[k + 1] + open_gap
            F = max(fe, fo)
            if F > cell:
                cell, sel = F, 3
            diag, H[k] = H[k], cell
            col[k] = (sel, 1 if ee > eo else 0, 1 if fe > fo else 0)
            if cell > best:
                best, bj, bk = cell, j, k
        dirs.append(col)

    def hsel(j, k):
        return 0 if j < 0 or j >= len(dirs) or k >= L else dirs[j][k][0]

    ops = []
    j, k, state = bj, bk, "H"
    while True:
        if state == "H":
            s = hsel(j, k)
            if s == 0:
                break
            if s == 1:
                ops.append("=" if int(db[end - j]) == qs[k] else "X")
                j, k = j - 1, k + 1
            else:
                state = "E" if s == 2 else "F"
        elif state == "E":
            ops.append("D")
            state = "E" if dirs[j][k][1] else "H"
            j -= 1
        else:
            ops.append("I")
            state = "F" if dirs[j][k][2] else "H"
            k += 1
    return dict(score=best, q_start=bk, q_end=k - 1, s_start=end - bj, s_end=end - j - 1, ops="".join(ops))


def runs(ops: str) -> list[int]:
    """The run-length words (length << 4 | op) of an operation string."""
    return [len(list(g)) << 4 | OPS.index(c) for c, g in itertools.groupby(ops)]


def expand(words) -> str:
    return "".join(OPS[int(w) & 3] * (int(w) >> 4) for w in words)


def hit_words(rec, ops, h):
    o = int(rec["ops_offset"][h])
    return ops[o:o + int(rec["n_runs"][h])]


# ---------------------------------------------------------------- invariants
def check_path(qs, db, M, r, words, open_gap, extend_gap, db_start=None, ext=None, aln=None):
    """The eight invariants on one hit. r: its record (absolute subject
    coordinates), words: its run-length words, db_start: the hit's known
    absolute start, ext: its GhostmHitExt (q_start, q_end, mismatches,
    gap_opens), aln: its (aln_len, aln_match). Returns the operation string."""
    M = M if isinstance(M, list) else [int(x) for x in M]
    for a, b in zip(words[:-1], words[1:]):
        assert (int(a) & 15) != (int(b) & 15) and int(a) >> 4 > 0  # maximal runs, ops 0..3
    assert all(int(w) & 12 == 0 and int(w) >> 4 > 0 for w in words)
    ops = expand(words)
    q, p, score, prev = int(r["q_start"]), int(r["s_start"]), 0, None
    for o in ops:
        if o in "=X":
            assert (o == "=") == (int(db[p]) == int(qs[q])), (q, p, o)         # 1
            score += M[int(db[p]) * 32 + int(qs[q])]
            q, p = q + 1, p + 1
        elif o == "D":
            score += extend_gap if prev == "D" else open_gap
            p += 1
        else:
            score += extend_gap if prev == "I" else open_gap
            q += 1
        prev = o
    n = {c: ops.count(c) for c in OPS}
    assert n["="] + n["X"] + n["I"] == int(r["q_end"]) - int(r["q_start"]) + 1 and q - 1 == int(r["q_end"])   # 2
    assert n["="] + n["X"] + n["D"] == int(r["s_end"]) - int(r["s_start"]) + 1 and p - 1 == int(r["s_end"])   # 3
    assert score == int(r["score"]) > 0, (score, int(r["score"]))                # 4
    assert ops[0] in "=X" and ops[-1] in "=X"                                    # 5
    gap_runs = [len(m.group()) for m in re.finditer(r"D+|I+", ops)]
    if db_start is not None:
        assert int(r["s_start"]) == int(db_start)                               # 6
    if ext is not None:
        e_qs, e_qe, e_mism, e_opens = (int(x) for x in ext)
        assert int(r["q_start"]) == e_qs                                        # 6
        mine = (len(ops), n["="], n["X"], len(gap_runs), int(r["q_end"]))
        if aln is not None:
            theirs = (int(aln[0]), int(aln[1]), e_mism, e_opens, e_qe)
            if e_opens == 0:
                assert not gap_runs and mine == theirs, (mine, theirs)          # 7
            if all(x == 1 for x in gap_runs):
                assert mine == theirs, (mine, theirs, ops)                      # 8
    return ops


def assert_gapped(rec, ops):
    """A set without gaps cannot pass silently: at least 20 hits with a gap in
    the CIGAR and at least 5 with a gap run of two or more."""
    gapped = long_runs = 0
    for h in range(len(rec)):
        w = hit_words(rec, ops, h)
        g = [int(x) >> 4 for x in w if int(x) & 2]
        gapped += bool(g)
        long_runs += any(x >= 2 for x in g)
    assert gapped >= 20 and long_runs >= 5, (gapped, long_runs)
    return gapped, long_runs


def dense_case(L, seed=11, n=60):
    """A denser indel set than the fixture, should it fall short: n reads of L
    with one to three planted indels of 1-4 residues; (qseq, db, qid, end)."""
    rnd = random.Random(seed)
    db, qseq, qid, end = [tx.END], [], [], []
    for i in range(n):
        subj = [rnd.choice(tx.AA) for _ in range(rnd.randint(L + 40, L + 120))]
        off = rnd.randint(5, 20)
        r = subj[off:off + L + 12]
        for _ in range(rnd.randint(1, 3)):
            p, m = rnd.randint(4, len(r) - 8), rnd.randint(1, 4)
            if rnd.random() < 0.5:
                del r[p:p + m]
            else:
                r[p:p] = [rnd.choice(tx.AA) for _ in range(m)]
        r = (r + [rnd.choice(tx.AA) for _ in range(L)])[:L]
        qseq.append(tx.codes("".join(r)))
        qid.append(i)
        end.append(len(db) + min(len(subj) - 1, off + L + 4))
        db += list(tx.codes("".join(subj))) + [tx.END]
    return (np.concatenate(qseq), np.array(db, dtype=np.uint8), np.array(qid, dtype=np.uint32),
            np.array(end, dtype=np.uint32))


RUNS = ("runs",)  # in place of the fixture's options: the hits of runs_hits


def runs_hits(root: str, L: int, base: int):
    """The compaction's boundary, (d, chunk, tb) like tx.fixture_hits, for the
    window `base` the caller will run: in one
    batch, hits of more than 64 run words (a read copied with every other
    residue replaced by its mildest mismatch: L runs of one column), of none (a
    read over W and C against a subject over D, E, N, K and R: every pair
    scores below zero, so the score is 0) and of one (an exact copy). The
    first hit is one of L words."""
    from ghostm_amd import traceback_path_host

    M = [int(x) for x in tx.blosum62()]
    rnd = random.Random(17)
    reads, subjects = [], []

    def near(a):  # the residue with the mildest score below zero against a
        return max((s, b) for s, b in ((M[tx.AA.index(b) * 32 + tx.AA.index(a)], b) for b in tx.AA) if s < 0)[1]

    for kind in (0, 1, 0, 2, 1, 0):
        if kind == 1:
            read = "".join(rnd.choice("WC") for _ in range(L))
            subj = "".join(rnd.choice("DENKR") for _ in range(L + 30))
        else:
            read = "".join(rnd.choice(tx.AA) for _ in range(L))
            subj = read if kind == 2 else "".join(near(a) if i % 2 else a for i, a in enumerate(read))
        reads.append(read)
        subjects.append(subj)
    d = os.path.join(root, f"tbpath_runs_L{L}")
    stamp = os.path.join(d, ".done")
    if not os.path.exists(stamp):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "db.fa"), "w") as f:
            f.write("".join(tx._fasta(f"s{i}", s) for i, s in enumerate(subjects)))
        with open(os.path.join(d, "q.fa"), "w") as f:
            f.write("".join(tx._fasta(f"r{i}", s) for i, s in enumerate(reads)))
        subprocess.run([tx.cases.GHOSTM, "db", "-i", f"{d}/db.fa", "-o", f"{d}/db"], check=True, capture_output=True)
        subprocess.run([tx.cases.GHOSTM, "qry", "-i", f"{d}/q.fa", "-o", f"{d}/q", "-l", str(L)], check=True,
                       capture_output=True)
        open(stamp, "w").close()
    chunk = tx.load_chunk(d)
    nq, L_, qseq, dbseq, pos = chunk
    assert (nq, L_) == (len(reads), L)
    for i, s in enumerate(subjects):
        assert np.array_equal(qseq[i * L:(i + 1) * L], tx.codes(reads[i]))
        assert np.array_equal(dbseq[int(pos[i]):int(pos[i]) + len(s)], tx.codes(s))
    qid = np.arange(nq, dtype=np.uint32)
    end = np.array([int(pos[i]) + len(s) - 1 for i, s in enumerate(subjects)], dtype=np.uint32)
    rec, _ = traceback_path_host(qseq, L, dbseq, tx.blosum62(), qid, end, base)
    n = [int(x) for x in rec["n_runs"]]
    assert n[0] > 64 and n[0] % 64 and 0 in n and 1 in n, n  # what the case is for
    tb = np.stack([qid, end, rec["s_start"].astype(np.uint32)], axis=1)
    return d, chunk, np.ascontiguousarray(tb)


# ---------------------------------------------------------------- stage level
def _recp(a):
    from ghostm_amd import native
    return a.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath))


def gpu_paths(lib, qid, end, starts, L, base, open_gap, extend_gap):
    """TraceBackPathGpu on the resident chunk: the size first (ops == NULL), then
    the words into a buffer with guard words behind them. Returns (rec, ops)."""
    from ghostm_amd import HIT_PATH_DTYPE, native

    n = len(qid)
    guard = 0xDEADBEEF
    rec = np.zeros(n + 1, dtype=HIT_PATH_DTYPE)
    rec["score"][n] = guard
    used = ctypes.c_size_t(12345)
    sp = None if starts is None else tx._p(starts)
    rc = lib.TraceBackPathGpu(n, tx._p(qid), tx._p(end), sp, L, base, open_gap, extend_gap, None, None, 0,
                              ctypes.byref(used))
    assert rc == 0, native.last_error()
    need = used.value
    ops = np.full(need + 4, guard, dtype=np.uint32)
    used2 = ctypes.c_size_t(12345)
    rc = lib.TraceBackPathGpu(n, tx._p(qid), tx._p(end), sp, L, base, open_gap, extend_gap, _recp(rec), tx._p(ops),
                              need, ctypes.byref(used2))
    assert rc == 0, native.last_error()
    assert used2.value == need
    assert (ops[need:] == guard).all() and rec["score"][n] == guard  # nothing past the last hit's words
    return rec[:n], ops[:need]


def stage_setup(lib, d, chunk, M):
    from ghostm_amd import native

    nq, L, qseq, dbseq, pos = chunk
    seed, kc, ipos = tx.load_index(d)
    M = np.ascontiguousarray(M, dtype=np.int32)
    assert lib.InitGpu() == 0
    assert lib.SetOptionGpu(1 << 27, M.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 0) == 0, native.last_error()
    assert lib.SetQueryGpu(tx._p(qseq, ctypes.c_uint8), nq, L) == 0, native.last_error()
    assert lib.SetDbGpu(tx._p(dbseq, ctypes.c_uint8), len(dbseq), tx._p(kc), len(kc), tx._p(ipos), len(ipos)) == 0


def stage_check(lib, d, chunk, tb, M, base, open_gap=-11, extend_gap=-1):
    """TraceBackPathGpu on the hits of tb, with and without the known starts, on
    60, 1 and 0 hits: record for record and word for word the host model's.
    Returns the host model's (rec, ops) of all hits."""
    from ghostm_amd import traceback_path_host

    nq, L, qseq, dbseq, pos = chunk
    stage_setup(lib, d, chunk, M)
    qid = np.ascontiguousarray(tb[:, 0])
    end = np.ascontiguousarray(tb[:, 1])
    starts = np.ascontiguousarray(tb[:, 2])
    want = traceback_path_host(qseq, L, dbseq, M, qid, end, base, open_gap, extend_gap)
    for count in (len(qid), 1, 0):
        for s_in in (None, np.ascontiguousarray(starts[:count])):
            w_rec, w_ops = traceback_path_host(qseq, L, dbseq, M, qid[:count], end[:count], base, open_gap,
                                               extend_gap, s_in)
            g_rec, g_ops = gpu_paths(lib, np.ascontiguousarray(qid[:count]), np.ascontiguousarray(end[:count]), s_in,
                                     L, base, open_gap, extend_gap)
            assert np.array_equal(g_rec, w_rec), (count, s_in is None)
            assert np.array_equal(g_ops, w_ops), (count, s_in is None)
            assert np.array_equal(w_rec, want[0][:count])  # the known starts change nothing
    assert lib.FreeGpu() == 0
    return want


# ---------------------------------------------------------------- session level
def session_expected(d, hits, inputs, M, base_of, open_gap=-11, extend_gap=-1):
    """The host model's (records, ops) of every session hit, from the formatted
    files: inputs[h] = (query chunk, local query, DB chunk, absolute end,
    absolute start) as tbext_cases.session_expected resolved them. Subject
    coordinates relative to the subject, the words in hit order."""
    from ghostm_amd import HIT_PATH_DTYPE, traceback_path_host

    qs, dbs = tx.dataset_chunks(d)
    want = np.zeros(len(hits), dtype=HIT_PATH_DTYPE)
    words = [None] * len(hits)
    groups = {}
    for h, (qi, q, di, end, start) in enumerate(inputs):
        groups.setdefault((qi, di), []).append(h)
    for (qi, di), idx in groups.items():
        L, qseq, dbseq = qs[qi][2], qs[qi][3], dbs[di][2]
        rec, ops = traceback_path_host(qseq, L, dbseq, M, [inputs[h][1] for h in idx], [inputs[h][3] for h in idx],
                                       base_of(L), open_gap, extend_gap, [inputs[h][4] for h in idx])
        for k, h in enumerate(idx):
            pos = inputs[h][4] - int(hits["db_start"][h])
            want[h] = rec[k]
            want["s_start"][h] -= pos
            want["s_end"][h] -= pos
            words[h] = hit_words(rec, ops, k)
    at = 0
    for h in range(len(hits)):
        want["ops_offset"][h] = at
        at += len(words[h])
    all_ops = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, dtype=np.uint32)
    return want, all_ops


def check_session_invariants(d, hits, ext, rec, ops, inputs, M, open_gap=-11, extend_gap=-1):
    qs, dbs = tx.dataset_chunks(d)
    Ml = [int(x) for x in M]
    for h, (qi, q, di, end, start) in enumerate(inputs):
        L = qs[qi][2]
        pos = start - int(hits["db_start"][h])
        r = dict(q_start=rec["q_start"][h], q_end=rec["q_end"][h], s_start=int(rec["s_start"][h]) + pos,
                 s_end=int(rec["s_end"][h]) + pos, score=rec["score"][h])
        check_path(qs[qi][3][q * L:(q + 1) * L], dbs[di][2], Ml, r, hit_words(rec, ops, h), open_gap, extend_gap,
                   db_start=start, ext=tuple(ext[h]), aln=(hits["aln_len"][h], hits["aln_match"][h]))
