"""Shared by tests/test_path_rows_host.py and tests/test_gpu_path_rows.py (not
a test module): a Python model of the aligned residue rows written from their
contract, the invariant checker, hand-made paths, the refused calls and the
stage- and session-level comparisons with the host model.

The contract (include/ghostm_hip.h, GhostmHitRows / PathRowsGpu): a hit is a
query record, its first query row, its first subject position (absolute in the
DB chunk) and run-length words length << 4 | op, ops = X I D. Column by column:
    = X   both letters; midline: the query letter for '=', '+' for an 'X' whose
          M[db code * 32 + query code] > 0, else a space
    I     the query letter over '-'; D: '-' over the subject letter; midline space
the letter of code c is "ARNDCQEGHILKMFPSTWYVBJZX*"[c], '?' from 25 up.
identities = '=' columns, positives = '=' and 'X' columns with a matrix entry
> 0, gap_residues = I and D columns, rescore = the pair columns' entries plus,
per I or D word, open_gap for its first column and extend_gap for the others."""
from __future__ import annotations

import ctypes
import os
import random
import subprocess

import numpy as np

import cases
import tbext_cases as tx
import tbpath_cases as tp

LETTERS = "ARNDCQEGHILKMFPSTWYVBJZX*"
GUARD = 0xEE


def letter(c: int) -> str:
    return LETTERS[c] if c < 25 else "?"


# ---------------------------------------------------------------- Python model
def rows_model(qs, db, M, q_start, s_start, words, open_gap=-11, extend_gap=-1):
    """One hit: dict(columns, identities, positives, gap_residues, rescore, q,
    mid, s); qs = the query record's codes, db = the chunk's residues."""
    q, p = int(q_start), int(s_start)
    rq, rm, rs = [], [], []
    ident = posit = gaps = score = 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 3
        for k in range(n):
            if op < 2:
                qc, sc = int(qs[q]), int(db[p])
                m = int(M[(sc & 31) * 32 + (qc & 31)])
                rq.append(letter(qc))
                rs.append(letter(sc))
                rm.append(letter(qc) if op == 0 else "+" if m > 0 else " ")
                ident += op == 0
                posit += m > 0
                score += m
                q, p = q + 1, p + 1
            else:
                rq.append(letter(int(qs[q])) if op == 2 else "-")
                rs.append(letter(int(db[p])) if op == 3 else "-")
                rm.append(" ")
                gaps += 1
                score += open_gap if k == 0 else extend_gap
                if op == 2:
                    q += 1
                else:
                    p += 1
    return dict(columns=len(rq), identities=ident, positives=posit, gap_residues=gaps, rescore=score,
                q="".join(rq).encode(), mid="".join(rm).encode(), s="".join(rs).encode())


def assert_equals_model(qseq, L, dbseq, M, qid, rec, ops, out, rows, open_gap, extend_gap):
    """Every record and every byte of (out, rows) against the Python model; the
    hits' bytes follow each other in hit order."""
    from ghostm_amd import rows_of

    at = 0
    Ml = [int(x) for x in M]
    for h in range(len(qid)):
        q = int(qid[h])
        m = rows_model(qseq[q * L:(q + 1) * L], dbseq, Ml, rec["q_start"][h], rec["s_start"][h],
                       tp.hit_words(rec, ops, h), open_gap, extend_gap)
        got = {f: int(out[f][h]) for f in ("columns", "identities", "positives", "gap_residues", "rescore")}
        assert got == {f: m[f] for f in got}, (h, got, m)
        assert int(out["query_record"][h]) == q and int(out["rows_offset"][h]) == at, h
        assert rows_of(out, rows, h) == (m["q"], m["mid"], m["s"]), h
        at += 3 * m["columns"]
    assert at == len(rows)


# ---------------------------------------------------------------- invariants
def check_rows(qs, subj, M, r, words, x, q, mid, s):
    """The invariants on one hit: r its path record (s_start indexing subj), x
    its rows record, (q, mid, s) its three rows. Returns the set of midline and
    gap kinds that occur: 'letter', '+', 'space', 'I', 'D'."""
    ops = tp.expand(words)
    n = {c: ops.count(c) for c in tp.OPS}
    assert int(x["rescore"]) == int(r["score"])
    assert int(x["columns"]) == len(ops) == len(q) == len(mid) == len(s)
    assert int(x["identities"]) == n["="] and int(x["gap_residues"]) == n["I"] + n["D"]
    q0, q1, s0, s1 = (int(r[f]) for f in ("q_start", "q_end", "s_start", "s_end"))
    assert q.replace(b"-", b"") == "".join(letter(int(c)) for c in qs[q0:q1 + 1]).encode()
    assert s.replace(b"-", b"") == "".join(letter(int(c)) for c in subj[s0:s1 + 1]).encode()
    kinds, posit = set(), 0
    a, b = q0, s0
    for c, o in enumerate(ops):
        ql, ml, sl = chr(q[c]), chr(mid[c]), chr(s[c])
        if o in "=X":
            m = int(M[int(subj[b]) * 32 + int(qs[a])])
            posit += m > 0
            want = ql if o == "=" else "+" if m > 0 else " "
            kinds.add("letter" if o == "=" else "+" if m > 0 else "space")
            assert (o == "=") == (ql == sl) and ql != "-" and sl != "-"
            a, b = a + 1, b + 1
        else:
            want = " "
            kinds.add(o)
            assert (ql, sl)[o == "I"] == "-" and (ql, sl)[o == "D"] != "-"
            a, b = a + (o == "I"), b + (o == "D")
        assert ml == want, (c, o, ml, want)
    assert int(x["positives"]) == posit
    return kinds


ALL_KINDS = {"letter", "+", "space", "I", "D"}


# ---------------------------------------------------------------- hand-made paths
def build_tiny(root: str):
    """A tiny chunk pair made with the formatters: 24 reads of 127 residues over
    six subjects of 60 to 90 residues (some B, Z, X and * among them). Returns
    (d, chunk)."""
    d = os.path.join(root, "pathrows_tiny")
    stamp = os.path.join(d, ".done")
    if not os.path.exists(stamp):
        os.makedirs(d, exist_ok=True)
        rnd = random.Random(17)
        alphabet = tx.AA * 3 + "BZX*"
        with open(os.path.join(d, "db.fa"), "w") as f:
            for i in range(6):
                f.write(f">s{i}\n" + "".join(rnd.choice(alphabet) for _ in range(rnd.randint(60, 90))) + "\n")
        with open(os.path.join(d, "q.fa"), "w") as f:
            for i in range(24):
                f.write(f">r{i}\n" + "".join(rnd.choice(alphabet) for _ in range(127)) + "\n")
        subprocess.run([cases.GHOSTM, "db", "-i", f"{d}/db.fa", "-o", f"{d}/db"], check=True, capture_output=True)
        subprocess.run([cases.GHOSTM, "qry", "-i", f"{d}/q.fa", "-o", f"{d}/q", "-l", "127"], check=True,
                       capture_output=True)
        open(stamp, "w").close()
    return d, tx.load_chunk(d)


def hand_paths(nq, L, db_len):
    """Paths no traceback would produce, at the shapes where a kernel with a
    lane per column breaks: (qid, rec, ops). The words lie in ops in another
    order than the hits, with unused words between them."""
    from ghostm_amd import HIT_PATH_DTYPE

    assert L == 127 and nq >= 8 and db_len >= 300
    E, X, I, D = 0, 1, 2, 3
    w = lambda n, op: n << 4 | op  # noqa: E731
    alt = lambda a, b, pairs: [w(1, a), w(1, b)] * pairs  # noqa: E731
    hits = [  # (query record, q_start, s_start, words)
        (0, 5, 9, []),                                        # 0 columns
        (1, 0, 1, [w(1, E)]),                                 # 1 column, at position 1 behind the leading END
        (2, 3, 7, [w(63, X)]),
        (3, 0, 40, [w(64, E)]),
        (4, 2, 11, [w(30, E), w(5, I), w(30, X)]),            # 65
        (5, 7, 100, [w(60, E), w(9, D), w(60, X)]),           # 129
        (6, 20, 150, [w(100, E)]),                            # one run longer than a wave
        (7, 0, 30, alt(E, I, 36)),                            # 72 runs of one column
        (0, 60, 20, alt(X, D, 40)),                           # 80 runs
        (1, 10, 60, alt(E, D, 65)),                           # 130 runs: two carries
        (2, 0, db_len - 50, [w(20, X), w(10, D), w(20, E)]),  # ends on the chunk's last residue
        (nq - 1, L - 36, 200, [w(30, E), w(2, I), w(3, I), w(4, D), w(1, I)]),  # the last record, to its last row
        (3, 126, 5, [w(1, I)]),                               # a lone gap column
        (nq - 1, 0, 1, [w(70, D), w(127, I)]),                # gaps only, longer than a wave
    ]
    rnd = random.Random(5)
    order = list(range(len(hits)))
    rnd.shuffle(order)
    ops, where = [], {}
    for h in order:
        ops += [0xFFFFFFFF] * rnd.randint(0, 3)  # never read: not a hit's words
        where[h] = len(ops)
        ops += hits[h][3]
    ops.append(0xFFFFFFFF)
    rec = np.zeros(len(hits), dtype=HIT_PATH_DTYPE)
    for h, (q, q0, s0, words) in enumerate(hits):
        rec[h] = (q0, 0, s0, 0, 0, len(words), where[h])
    return (np.array([x[0] for x in hits], dtype=np.uint32), rec, np.array(ops, dtype=np.uint32))


HAND_COLUMNS = [0, 1, 63, 64, 65, 129, 100, 72, 80, 130, 50, 40, 1, 197]


# ---------------------------------------------------------------- calls
def _recp(a):
    from ghostm_amd import native
    return a.ctypes.data_as(ctypes.POINTER(native.GhostmHitPath))


def _outp(a):
    from ghostm_amd import native
    return a.ctypes.data_as(ctypes.POINTER(native.GhostmHitRows))


def host_call(lib, chunk, M, open_gap=-11, extend_gap=-1):
    """call(qid, rec, ops, ops_len, out, rows, cap, used) -> rc for GhostmPathRowsHost on chunk."""
    nq, L, qseq, dbseq, pos = chunk
    Mi = np.ascontiguousarray(M, dtype=np.int32)

    def call(qid, rec, ops, ops_len, out, rows, cap, used):
        return lib.GhostmPathRowsHost(
            tx._p(qseq, ctypes.c_uint8), nq, L, tx._p(dbseq, ctypes.c_uint8), len(dbseq),
            Mi.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(qid), tx._p(qid), _recp(rec), tx._p(ops), ops_len, L,
            open_gap, extend_gap, None if out is None else _outp(out),
            None if rows is None else tx._p(rows, ctypes.c_uint8), cap, ctypes.byref(used))
    return call


def gpu_call(lib, L, open_gap=-11, extend_gap=-1):
    """The same for PathRowsGpu on the resident chunk (tp.stage_setup)."""
    def call(qid, rec, ops, ops_len, out, rows, cap, used):
        return lib.PathRowsGpu(len(qid), tx._p(qid), _recp(rec), tx._p(ops), ops_len, L, open_gap, extend_gap,
                               None if out is None else _outp(out),
                               None if rows is None else tx._p(rows, ctypes.c_uint8), cap, ctypes.byref(used))
    return call


def rows_via(call, qid, rec, ops):
    """The size first (rows == NULL, out == NULL), then the counts alone, then
    the bytes into a buffer with guard bytes behind them. Returns (out, rows)."""
    from ghostm_amd import HIT_ROWS_DTYPE, native

    qid = np.ascontiguousarray(qid, dtype=np.uint32)
    rec = np.ascontiguousarray(rec)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    n = len(qid)
    used = ctypes.c_size_t(12345)
    assert call(qid, rec, ops, len(ops), None, None, 0, used) == 0, native.last_error()
    need = used.value
    counts = np.zeros(n + 1, dtype=HIT_ROWS_DTYPE)
    used = ctypes.c_size_t(12345)
    assert call(qid, rec, ops, len(ops), counts, None, 0, used) == 0, native.last_error()
    assert used.value == need
    out = np.zeros(n + 1, dtype=HIT_ROWS_DTYPE)
    out["rescore"][n] = -77
    rows = np.full(need + 64, GUARD, dtype=np.uint8)
    used = ctypes.c_size_t(12345)
    assert call(qid, rec, ops, len(ops), out, rows, need, used) == 0, native.last_error()
    assert used.value == need
    assert (rows[need:] == GUARD).all() and out["rescore"][n] == -77  # nothing past the last hit
    assert np.array_equal(counts[:n], out[:n])
    assert need == 3 * int(out["columns"][:n].sum())
    return out[:n], rows[:need]


def refusal_cases(nq, L, db_len):
    """(reason, qid, rec, ops, ops_len, rows_cap): one call per reason the
    contract names, each a well-formed call with one thing wrong."""
    from ghostm_amd import HIT_PATH_DTYPE

    def one(q=0, q0=0, s0=1, words=(10 << 4,), ops_len=None, cap=1 << 20, offset=0):
        rec = np.zeros(2, dtype=HIT_PATH_DTYPE)
        rec[0] = (0, 0, 1, 0, 0, 1, 0)  # a good first hit: 10=
        rec[1] = (q0, 0, s0, 0, 0, len(words), 1 + offset)
        ops = np.array([10 << 4] + list(words), dtype=np.uint32)
        return (np.array([0, q], dtype=np.uint32), rec, ops, len(ops) if ops_len is None else ops_len, cap)

    return [
        ("ops", *one(ops_len=1)),
        ("ops", *one(offset=1)),
        ("word", *one(words=(10 << 4 | 4,))),
        ("word", *one(words=(10 << 4 | 8,))),
        ("word", *one(words=(3,))),                       # length 0
        ("bounds", *one(q0=L - 9)),                       # ten query residues from L - 9
        ("bounds", *one(s0=db_len - 9)),
        ("bounds", *one(q0=L - 4, words=(5 << 4 | 2,))),  # an insertion consumes query residues
        ("bounds", *one(s0=db_len - 4, words=(5 << 4 | 3,))),
        ("query", *one(q=nq)),
        ("rows_cap", *one(cap=59)),                       # 60 bytes needed
    ]


def check_refusals(call, nq, L, db_len):
    from ghostm_amd import HIT_ROWS_DTYPE, native

    seen = set()
    for reason, qid, rec, ops, ops_len, cap in refusal_cases(nq, L, db_len):
        out = np.zeros(2, dtype=HIT_ROWS_DTYPE)
        out.view(np.uint8)[:] = GUARD
        rows = np.full(256, GUARD, dtype=np.uint8)
        used = ctypes.c_size_t(4242)
        rc = call(qid, rec, ops, ops_len, out, rows, cap, used)
        assert rc != 0 and reason in native.last_error(), (reason, rc, native.last_error())
        assert (out.view(np.uint8) == GUARD).all() and (rows == GUARD).all() and used.value == 4242, reason
        seen.add(reason)
    assert seen == {"ops", "word", "bounds", "query", "rows_cap"}
    # the limits themselves are fine: the last row, the last residue, the exact capacity
    from ghostm_amd import HIT_PATH_DTYPE
    rec = np.zeros(1, dtype=HIT_PATH_DTYPE)
    rec[0] = (L - 10, 0, db_len - 10, 0, 0, 1, 0)
    out = np.zeros(1, dtype=HIT_ROWS_DTYPE)
    rows = np.full(31, GUARD, dtype=np.uint8)
    used = ctypes.c_size_t(0)
    assert call(np.array([nq - 1], dtype=np.uint32), rec, np.array([10 << 4], dtype=np.uint32), 1, out, rows, 30,
                used) == 0, native.last_error()
    assert used.value == 30 and rows[30] == GUARD and (rows[:30] != GUARD).all()


# ---------------------------------------------------------------- fixture paths
def fixture_paths(root, L, matrix="blosum62", gaps=(-11, -1)):
    """The indel fixture at L with the host model's paths of the oracle's 60
    hits: (d, chunk, M, qid, rec, ops); rec.s_start absolute in the chunk."""
    from ghostm_amd import traceback_path_host

    opts = () if matrix == "blosum62" else ("-M", cases.PAM250, "-G", str(-gaps[0]), "-E", str(-gaps[1]))
    d, chunk, tb = tx.fixture_hits(root, L, opts)
    nq, L_, qseq, dbseq, pos = chunk
    M = tx.blosum62() if matrix == "blosum62" else tx.pam250()
    rec, ops = traceback_path_host(qseq, L, dbseq, M, tb[:, 0], tb[:, 1], L + 2 * 2 * 2 * 16, gaps[0], gaps[1])
    return d, chunk, M, np.ascontiguousarray(tb[:, 0]), rec, ops


def stage_check(lib, d, chunk, M, qid, rec, ops, open_gap=-11, extend_gap=-1, counts=None):
    """PathRowsGpu on the first 60 (all), 1 and 0 hits of (qid, rec, ops) on the
    chunk made resident here: record for record and byte for byte the host
    model's, guard bytes intact (rows_via). Returns the hits checked."""
    tp.stage_setup(lib, d, chunk, M)
    host, gpu = host_call(lib, chunk, M, open_gap, extend_gap), gpu_call(lib, chunk[1], open_gap, extend_gap)
    done = 0
    for count in counts or (len(qid), 1, 0):
        w_out, w_rows = rows_via(host, qid[:count], rec[:count], ops)
        g_out, g_rows = rows_via(gpu, qid[:count], rec[:count], ops)
        assert np.array_equal(g_out, w_out), count
        assert np.array_equal(g_rows, w_rows), count
        done += count
    assert lib.FreeGpu() == 0
    return done


# ---------------------------------------------------------------- session level
def session_rows_expected(d, hits, inputs, rec, ops, M, open_gap=-11, extend_gap=-1):
    """The host model applied to a session's hits_path(): (records, rows) in hit
    order. inputs[h] = (query chunk, local query, DB chunk, absolute end,
    absolute start) as tbext_cases.session_expected resolved them."""
    from ghostm_amd import HIT_ROWS_DTYPE, path_rows_host, rows_of

    qs, dbs = tx.dataset_chunks(d)
    want = np.zeros(len(hits), dtype=HIT_ROWS_DTYPE)
    parts = [b""] * len(hits)
    groups = {}
    for h, (qi, q, di, end, start) in enumerate(inputs):
        groups.setdefault((qi, di), []).append(h)
    for (qi, di), idx in groups.items():
        L, qseq, dbseq = qs[qi][2], qs[qi][3], dbs[di][2]
        r = rec[idx].copy()
        for k, h in enumerate(idx):
            pos = inputs[h][4] - int(hits["db_start"][h])
            r["s_start"][k] += pos
            r["s_end"][k] += pos
        out, rows = path_rows_host(qseq, L, dbseq, M, [inputs[h][1] for h in idx], r, ops, open_gap, extend_gap)
        for k, h in enumerate(idx):
            want[h] = out[k]
            want["query_record"][h] = qs[qi][0] + inputs[h][1]
            parts[h] = b"".join(rows_of(out, rows, k))
    at = 0
    for h in range(len(hits)):
        want["rows_offset"][h] = at
        at += len(parts[h])
    return want, np.frombuffer(b"".join(parts), dtype=np.uint8)
