"""Shared by tests/test_pileup_host.py, tests/test_gpu_pileup.py and
tests/pileup_poison_child.py (not a test module): a numpy model of the subject
pile-up written from its contract, the calls, the refused calls, the smallest
shapes at which a tiled kernel breaks and the stage- and session-level
comparisons.

The contract (include/ghostm_hip.h, above PathPileupGpu): with slot(c) = c for
c < 25 and 25 otherwise, a '=' or 'X' column at subject position p adds 1 to
profile[p][slot(query code)], a 'D' column adds 1 to profile[p][26], an 'I'
column adds nothing; depth = the sum of slots 0..26, identities =
profile[p][slot(db[p])], consensus = the first largest of slots 0..24, 255 when
they are all zero. Everything is integer, so every comparison is equality."""
from __future__ import annotations

import ctypes

import numpy as np

import pathrows_cases as pr
import tbext_cases as tx
import tbpath_cases as tp

GUARD32 = 0xEEEEEEEE
GUARD8 = 0xEE
PAD = 8  # guard elements behind every output


# ---------------------------------------------------------------- numpy model
def finish(prof, dbseq):
    """(depth, identities, consensus) of a profile (n, 32) over residues dbseq."""
    n = len(dbseq)
    depth = prof[:, :27].sum(axis=1, dtype=np.uint64).astype(np.uint32)
    ident = prof[np.arange(n), np.minimum(np.asarray(dbseq, dtype=np.int64), 25)]
    head = prof[:, :25]
    cons = np.where(head.max(axis=1, initial=0) > 0, head.argmax(axis=1), 255).astype(np.uint8) if n else \
        np.zeros(0, dtype=np.uint8)
    return depth, ident.astype(np.uint32), cons


def add_path(P, S, codes, q_start, s_start, words):
    """Appends the (position, slot) pairs of one path to the lists P and S;
    codes = the query record's codes, s_start = the first position."""
    q, s = int(q_start), int(s_start)
    for w in words:
        n, op = int(w) >> 4, int(w) & 3
        if op < 2:
            P.append(np.arange(s, s + n))
            S.append(np.minimum(np.asarray(codes[q:q + n], dtype=np.int64), 25))
            q, s = q + n, s + n
        elif op == 2:
            q += n
        else:
            P.append(np.arange(s, s + n))
            S.append(np.full(n, 26, dtype=np.int64))
            s += n


def model(qseq, L, dbseq, qid, rec, ops):
    """(depth, identities, consensus, profile) of hits on a chunk."""
    prof = np.zeros((len(dbseq), 32), dtype=np.uint32)
    P, S = [], []
    for h in range(len(qid)):
        q = int(qid[h])
        add_path(P, S, qseq[q * L:(q + 1) * L], rec["q_start"][h], rec["s_start"][h], tp.hit_words(rec, ops, h))
    if P:
        np.add.at(prof, (np.concatenate(P), np.concatenate(S)), 1)
    return (*finish(prof, dbseq), prof)


# ---------------------------------------------------------------- calls
def host_call(lib, chunk):
    """call(qid, rec, ops, ops_len, db_len, depth, ident, cons, prof) -> rc for
    GhostmPathPileupHost on chunk (db_len only chooses the output sizes)."""
    nq, L, qseq, dbseq, pos = chunk

    def call(qid, rec, ops, ops_len, db_len, depth, ident, cons, prof):
        return lib.GhostmPathPileupHost(
            tx._p(qseq, ctypes.c_uint8), nq, L, tx._p(dbseq, ctypes.c_uint8), len(dbseq), None, len(qid), tx._p(qid),
            pr._recp(rec), tx._p(ops), ops_len, L, None if depth is None else tx._p(depth),
            None if ident is None else tx._p(ident), None if cons is None else tx._p(cons, ctypes.c_uint8),
            None if prof is None else tx._p(prof))
    return call


def gpu_call(lib, L):
    """The same for PathPileupGpu on the resident chunk (tp.stage_setup)."""
    def call(qid, rec, ops, ops_len, db_len, depth, ident, cons, prof):
        return lib.PathPileupGpu(
            len(qid), tx._p(qid), pr._recp(rec), tx._p(ops), ops_len, L, db_len, None if depth is None else tx._p(depth),
            None if ident is None else tx._p(ident), None if cons is None else tx._p(cons, ctypes.c_uint8),
            None if prof is None else tx._p(prof))
    return call


def guarded(db_len, profile=True):
    return (np.full(db_len + PAD, GUARD32, dtype=np.uint32), np.full(db_len + PAD, GUARD32, dtype=np.uint32),
            np.full(db_len + PAD, GUARD8, dtype=np.uint8),
            np.full((db_len + PAD) * 32, GUARD32, dtype=np.uint32) if profile else None)


def pileup_via(call, qid, rec, ops, db_len, profile=True):
    """One call into guard-filled outputs; nothing is written behind db_len
    elements. Returns (depth, identities, consensus, profile or None)."""
    from ghostm_amd import native

    qid = np.ascontiguousarray(qid, dtype=np.uint32)
    rec = np.ascontiguousarray(rec)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    depth, ident, cons, prof = guarded(db_len, profile)
    assert call(qid, rec, ops, len(ops), db_len, depth, ident, cons, prof) == 0, native.last_error()
    assert (depth[db_len:] == GUARD32).all() and (ident[db_len:] == GUARD32).all() and (cons[db_len:] == GUARD8).all()
    if profile:
        assert (prof[db_len * 32:] == GUARD32).all()
        prof = prof[:db_len * 32].reshape(db_len, 32)
    return depth[:db_len], ident[:db_len], cons[:db_len], prof


def assert_same(got, want, what):
    for name, g, w in zip(("depth", "identities", "consensus", "profile"), got, want):
        if g is None:
            continue
        bad = np.nonzero(np.asarray(g) != np.asarray(w))
        assert len(bad[0]) == 0, (what, name, [b[:5].tolist() for b in bad])


def check_against_model(call, chunk, qid, rec, ops, what):
    """With the profile and without it against the numpy model. Returns the
    model's arrays."""
    nq, L, qseq, dbseq, pos = chunk
    want = model(qseq, L, dbseq, qid, rec, ops)
    assert_same(pileup_via(call, qid, rec, ops, len(dbseq), True), want, what)
    assert_same(pileup_via(call, qid, rec, ops, len(dbseq), False), want, what)
    assert (want[3][:, 27:] == 0).all() and np.array_equal(want[0], want[3].sum(axis=1))
    return want


# ---------------------------------------------------------------- refusals
def check_refusals(call, nq, L, db_len, gpu):
    """Every refusal names its reason and leaves guard-filled outputs as they
    were. db_len (not the resident chunk's length) exists on the device only."""
    from ghostm_amd import native

    seen = set()
    todo = [(r, q, rec, ops, n, db_len, False) for r, q, rec, ops, n, cap in pr.refusal_cases(nq, L, db_len)
            if r != "rows_cap"]
    good = pr.refusal_cases(nq, L, db_len)[0]
    ok_q, ok_rec, ok_ops = good[1][:1], good[2][:1], good[3]  # its first hit alone is well formed
    if gpu:
        todo.append(("db_len", ok_q, ok_rec, ok_ops, len(ok_ops), db_len - 1, False))
        todo.append(("db_len", ok_q, ok_rec, ok_ops, len(ok_ops), db_len + 1, False))
    todo.append(("null", ok_q, ok_rec, ok_ops, len(ok_ops), db_len, True))
    for reason, qid, rec, ops, ops_len, dl, null in todo:
        depth, ident, cons, prof = guarded(db_len + 1)
        rc = call(qid, rec, ops, ops_len, dl, None if null else depth, ident, cons, prof)
        assert rc != 0 and reason in native.last_error(), (reason, rc, native.last_error())
        assert (depth == GUARD32).all() and (ident == GUARD32).all() and (cons == GUARD8).all() and \
            (prof == GUARD32).all(), reason
        seen.add(reason)
    assert seen == {"ops", "word", "bounds", "query", "null"} | ({"db_len"} if gpu else set())
    # the limits themselves are fine: the last row and the chunk's last residue
    from ghostm_amd import HIT_PATH_DTYPE
    rec = np.zeros(1, dtype=HIT_PATH_DTYPE)
    rec[0] = (L - 10, 0, db_len - 10, 0, 0, 1, 0)
    d = pileup_via(call, np.array([nq - 1], dtype=np.uint32), rec, np.array([10 << 4], dtype=np.uint32), db_len)[0]
    assert d[db_len - 10:].tolist() == [1] * 10 and int(d.sum()) == 10


# ---------------------------------------------------------------- the smallest shapes that can break
EDGE_ENV = {"GHOSTM_PILEUP_TILE": "32", "GHOSTM_PILEUP_PART_HITS": "7"}


def edge_cases(nq, L, db_len):
    """name -> (qid, rec, ops), for tiles of 32 positions and parts of 7 hits."""
    from ghostm_amd import HIT_PATH_DTYPE

    assert L == 127 and nq >= 8 and db_len >= 300
    E, X, I, D = 0, 1, 2, 3
    w = lambda n, op: n << 4 | op  # noqa: E731

    def make(hits):
        ops, rec = [], np.zeros(len(hits), dtype=HIT_PATH_DTYPE)
        for h, (q, q0, s0, words) in enumerate(hits):
            rec[h] = (q0, 0, s0, 0, 0, len(words), len(ops))
            ops += words
        return np.array([x[0] for x in hits], dtype=np.uint32), rec, np.array(ops + [0xFFFFFFFF], dtype=np.uint32)

    three = (0, 3, 40, [w(30, E), w(40, X)])                   # positions 40..109: tiles 1, 2 and 3
    d_edge = (1, 0, 50, [w(10, E), w(10, D), w(10, X)])        # the D run covers 60..69, over the edge at 64
    i_edge = (2, 5, 54, [w(10, E), w(5, I), w(10, E)])         # 54..63, an insertion, then 64..73
    first = (3, 0, 1, [w(1, E)])                               # position 1 behind the leading END
    last = (4, 2, db_len - 50, [w(20, X), w(10, D), w(20, E)])  # ends on the chunk's last residue
    ends_on_edge = (5, 0, 20, [w(12, E)])                      # 20..31: ends on a tile's last position
    starts_on_edge = (6, 9, 96, [w(3, D), w(5, E)])            # starts on a tile's first position with a deletion
    one = (7, 60, 70, [w(20, E)])                              # inside tile 2
    mixed = [three, d_edge, i_edge, first, last, ends_on_edge, starts_on_edge, one, (0, 5, 9, [])]
    return {
        "three_tiles": make([three]),
        "d_across_edge": make([d_edge]),
        "i_at_edge": make([i_edge]),
        "position_1": make([first]),
        "last_residue": make([last]),
        "tile_ends": make([ends_on_edge, starts_on_edge]),
        "copies_300": make([one] * 300),                       # counts pass 255; the tile's list splits into 43 parts
        "mixed": make(mixed),
        "mixed_reversed": make(mixed[::-1]),
    }


def stage_check(lib, d, chunk, M, qid, rec, ops, counts=None, edges=False):
    """PathPileupGpu on the chunk made resident here against the numpy model and
    the host model: the first 60 (all), 1 and 0 hits, with and without the
    profile. Returns the hits checked."""
    tp.stage_setup(lib, d, chunk, M)
    host, gpu = host_call(lib, chunk), gpu_call(lib, chunk[1])
    done = 0
    for count in counts or (len(qid), 1, 0):
        want = check_against_model(host, chunk, qid[:count], rec[:count], ops, ("host", count))
        got = check_against_model(gpu, chunk, qid[:count], rec[:count], ops, ("gpu", count))
        assert_same(got, want, count)
        done += count
    if edges:
        nq, L, qseq, dbseq, pos = chunk
        with pr_env(EDGE_ENV):
            for name, (q, r, o) in edge_cases(nq, L, len(dbseq)).items():
                want = check_against_model(gpu, chunk, q, r, o, name)
                if name == "copies_300":
                    assert int(want[0].max()) == 300 and int(want[3].max()) == 300
                done += len(q)
    assert lib.FreeGpu() == 0
    return done


class pr_env:
    """Sets environment variables for a block."""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- session level
def subject_layout(d):
    """Per subject in db_id order: (DB chunk, first position in the chunk,
    length), and the subjects' offsets in the concatenated arrays."""
    qs, dbs = tx.dataset_chunks(d)
    subj = []
    for di, (base, nsub, dbseq, pos) in enumerate(dbs):
        for s in range(nsub):
            nxt = int(pos[s + 1]) if s + 1 < nsub else len(dbseq)
            subj.append((di, int(pos[s]), nxt - int(pos[s]) - 1))
            assert dbseq[nxt - 1] == 25 and (dbseq[int(pos[s]):nxt - 1] != 25).all()  # one END behind every subject
    off = np.concatenate([[0], np.cumsum([x[2] for x in subj])]).astype(np.int64)
    return qs, dbs, subj, off


def session_model(d, hits, query_record, rec, ops):
    """The numpy model applied to a session's hits_path(): hit h lies in global
    query record query_record[h] (hits_rows()) and on subject hits['db_id'][h],
    rec['s_start'] relative to the subject. Returns (subjects, depth,
    identities, consensus, profile) over the concatenated subjects."""
    from ghostm_amd import SUBJECT_PILEUP_DTYPE

    qs, dbs, subj, off = subject_layout(d)
    total = int(off[-1])
    residues = np.concatenate([dbs[di][2][p:p + n] for di, p, n in subj]) if subj else np.zeros(0, dtype=np.uint8)
    bases = [q[0] for q in qs]
    prof = np.zeros((total, 32), dtype=np.uint32)
    P, S = [], []
    for h in range(len(hits)):
        g = int(query_record[h])
        qi = int(np.searchsorted(bases, g, side="right") - 1)
        L = qs[qi][2]
        local = g - qs[qi][0]
        add_path(P, S, qs[qi][3][local * L:(local + 1) * L], rec["q_start"][h],
                 int(off[int(hits["db_id"][h])]) + int(rec["s_start"][h]), tp.hit_words(rec, ops, h))
    if P:
        np.add.at(prof, (np.concatenate(P), np.concatenate(S)), 1)
    depth, ident, cons = finish(prof, residues)
    want = np.zeros(len(subj), dtype=SUBJECT_PILEUP_DTYPE)
    nhits = np.bincount(hits["db_id"], minlength=len(subj))
    for i, (di, p, n) in enumerate(subj):
        a, b = int(off[i]), int(off[i + 1])
        want[i] = (n, nhits[i], int((depth[a:b] > 0).sum()), int(depth[a:b].max(initial=0)),
                   int(depth[a:b].sum(dtype=np.uint64)), int(ident[a:b].sum(dtype=np.uint64)), a)
    return want, depth, ident, cons, prof
