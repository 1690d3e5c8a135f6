"""Shared by tests/test_dp_model.py and tests/test_gpu_dp_edges.py (not a test
module): a plain int64 numpy model of the score DP (K2) and the traceback
(K3) written from their contract, the fixtures that put real values next to
every layout and encoding bound of the two kernels, and the generated matrices.

The contract is the reference's CalculateScoreCpu (aligner.cpp:545-685) and
TraceBack (aligner.cpp:771-949); oracle/ghostm_oracle.cpp Score and TraceBack
restate them one candidate at a time. The model here runs every candidate of a
fixture at once: the loops are over columns and rows only.

Where each bound comes from (ghostm_amd/csrc/device.hip, L = 127, gaps -11/-1)
-------------------------------------------------------------------------------
With hmax = bound = L * max|M|:

ScoreLaunch, score window base = L + 36 = 163, layout (32, 4), sigma_max =
(base + 2 G) * -ext = 171:
  integer patterns (swar): swar_top = 1100 + 2 * (171 + bound) + 32 + 10 + 32
      = 1516 + 2 * bound < 0x7C00 = 31744  <=>  bound <= 15113  <=>  m <= 119
      (m = 118: top 31488; m = 119: top 31742; m = 120: 31996, framed f16)
  framed f16 guard: bound + 171 < 2040 <=> m <= 14; from m = 15 the guard is
      2040 - 171 = 1869 (a swar launch has no guard, so the guard shows only
      from m = 120, or with GHOSTM_K2=f16frame)
  plain f16 guard (GHOSTM_K2=f16plain): bound < 2048 <=> m <= 16
  packed at all (ScorePacked): bound < 30000 <=> m <= 236; m = 237 runs int32
  framed at all: sigma_max <= 1000 <=> -ext <= 5 (171 * 6 = 1026)
  packed gaps: -open < 2000

LaunchTraceback, window base = L + 128 = 255 (span = Lpad + base = 383) and the
wide one L + 512 = 639 (-r 64, span 767):
  16-bit key DP: span < 500 and hmax < 8000 <=> m <= 62 (63 * 127 = 8001)
  17-bit key DP (wide window): span < 1000 and hmax < 4000 <=> m <= 31
  half (f16) scan: hmax < 2048 <=> m <= 16
  framed scan: hmax + (base + 2 G) * -ext < 2048: 263 at base 255 <=> m <= 14
  key frame: kframe = hmax + (span + 1) * -ext < 8000 (16-bit key); with
      diag(11), hmax = 1397 and span + 1 = 384: -ext = 17 gives 7925 (framed),
      -ext = 18 gives 8309 (unframed)
m = 11 is BLOSUM62's own scale, the baseline below every step.
"""
from __future__ import annotations

import functools
import os
import random
import subprocess

import numpy as np

import cases
import tbext_cases as tx

AA = tx.AA
END = 25
X = 23

# both ends of every (S, G) range of ChooseLayout
WIDTHS = [1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64, 65, 72, 73, 80, 81, 96, 97, 112, 113, 127]
# the (S, G) ChooseLayout must give for these widths, at the score window and both traceback windows
LAYOUTS = {(1, 8): (8, 1), (9, 16): (16, 1), (17, 24): (8, 3), (25, 32): (32, 1), (33, 40): (8, 5), (41, 48): (16, 3),
           (49, 56): (8, 7), (57, 64): (32, 2), (65, 72): (8, 9), (73, 80): (16, 5), (81, 96): (32, 3),
           (97, 112): (16, 7), (113, 127): (32, 4)}
SEED_K = 3          # db -k 3: the seed span; K1 seeds from this width on
THRESHOLD = 1       # aln -t 1: every occupied diagonal bin is a candidate
K2_WIDTHS = [L for L in WIDTHS if L >= SEED_K]
# diag(m) scales on each side of every encoding step (see the module docstring), and 119, the last swar scale
SCALES = [11, 14, 15, 16, 17, 31, 32, 62, 63, 118, 119, 120, 236, 237]
SWEEP_WIDTHS = [127, 100, 40]   # S = 32, S = 16, S = 8
# gap pairs on each side of: the frame limit, the packed limit, the key frame's field test
GAPS = [(-11, -1), (0, 0), (-11, -5), (-11, -6), (-1999, -1), (-2000, -1), (-18, -17), (-18, -18)]


def expected_layout(L: int):
    for (lo, hi), sg in LAYOUTS.items():
        if lo <= L <= hi:
            return sg
    raise ValueError(L)


def choose_layout(L: int, width: int):
    """ChooseLayout (device.hip) restated: the (S, G) with the fewest lane-steps per useful cell."""
    best, best_cost = (32, 1), 1e300
    for S in (32, 16, 8):
        G = (L + S - 1) // S
        if G == 0 or G > 16:
            continue
        gpw = 64 // G
        cost = float(G * S) * float(width + G - 1) / float(gpw * G)
        if cost < best_cost * 0.999:
            best_cost, best = cost, (S, G)
    return best


# ---------------------------------------------------------------- the model
def score_model(qseq, L, db, M, qid, start, base, extend, open_gap, ext_gap, detail=False):
    """(score, end) of every candidate (qid, start): local Gotoh score of the
    padded query against the window off = max(start - extend, 0), width base,
    clipped at the DB's end. An END column zeroes H and E; M[db * 32 + query];
    F uses this column's H[k - 1]; end = the last column with a cell >= best.
    detail: also a dict of per-candidate facts about the window: ties (earlier
    columns that reached the final, positive best), ends (its END columns),
    clipped_lo / clipped_hi (cut at the DB's start / end)."""
    M2 = np.asarray(M, dtype=np.int64).reshape(32, 32)
    QT = np.ascontiguousarray(np.asarray(qseq).reshape(-1, L)[np.asarray(qid, dtype=np.int64)].T).astype(np.int64)
    n = QT.shape[1]
    db = np.asarray(db).astype(np.int64)
    off = np.maximum(np.asarray(start, dtype=np.int64) - extend, 0)
    width = np.minimum(base, len(db) - off)
    dbp = np.concatenate([db, np.full(base, END, dtype=np.int64)])
    H = np.zeros((L + 1, n), dtype=np.int64)
    E = np.zeros((L + 1, n), dtype=np.int64)
    best = np.zeros(n, dtype=np.int64)
    end_col = np.zeros(n, dtype=np.int64)
    ties = np.zeros(n, dtype=np.int64)
    ends = np.zeros(n, dtype=np.int64)
    for j in range(base):
        inside = j < width
        c = dbp[off + j]
        is_end = inside & (c == END)
        ends += is_end
        live = inside & ~is_end
        H[:, is_end] = 0
        E[:, is_end] = 0
        S = M2[c[None, :], QT]                                   # row k - 1: M[c][q[k - 1]]
        En = np.maximum(E[1:] + ext_gap, H[1:] + open_gap)       # from the previous column
        T = np.maximum(np.maximum(H[:-1] + S, 0), En)
        Hn = np.zeros_like(H)
        F = np.zeros(n, dtype=np.int64)
        for k in range(1, L + 1):
            F = np.maximum(F + ext_gap, Hn[k - 1] + open_gap)    # this column's H[k - 1]
            Hn[k] = np.maximum(T[k - 1], F)
        colmax = Hn[1:].max(axis=0)
        upd = live & (colmax >= best)
        ties = np.where(live & (colmax > best), 0, ties + (upd & (best > 0)))
        best = np.where(upd, colmax, best)
        end_col = np.where(upd, j, end_col)
        H = np.where(live, Hn, H)
        E[1:] = np.where(live, En, E[1:])
    if detail:
        start = np.asarray(start, dtype=np.int64)
        return best, off + end_col, dict(ties=ties, ends=ends, clipped_lo=start < extend,
                                         clipped_hi=off + base > len(db))
    return best, off + end_col


def trace_model(qseq, L, db, M, qid, end, base, open_gap, ext_gap):
    """(start, len, match) of every hit (qid, end): the reverse DP over columns
    end, end - 1, ... (width end + 1 when end < base, else base), broken at END,
    rows L - 1 .. 0; strict > in that order picks the first maximum; (len,
    match) of a cell come from the H cell it steps from. base may be a tuple of
    windows: the DP is the same up to each window's last column, so one pass
    keeps one running maximum per window and returns one triple per window."""
    bases = base if isinstance(base, tuple) else (base,)
    M2 = np.asarray(M, dtype=np.int64).reshape(32, 32)
    QT = np.ascontiguousarray(np.asarray(qseq).reshape(-1, L)[np.asarray(qid, dtype=np.int64)].T).astype(np.int64)
    n = QT.shape[1]
    db = np.asarray(db).astype(np.int64)
    end = np.asarray(end, dtype=np.int64)
    widths = [np.where(end < b, end + 1, b) for b in bases]
    H = np.zeros((L + 1, n), dtype=np.int64)
    E = np.zeros((L + 1, n), dtype=np.int64)
    AM = np.zeros((L + 1, n), dtype=np.int64)
    AL = np.zeros((L + 1, n), dtype=np.int64)
    # per window: best, its column, its matches, its length
    best = [[np.zeros(n, dtype=np.int64) for _ in range(4)] for _ in bases]
    alive = np.ones(n, dtype=bool)
    cols = np.arange(n)
    for j in range(max(int(w.max()) for w in widths) if n else 0):
        c = db[np.maximum(end - j, 0)]
        alive = alive & (c != END) & (j <= end)
        if not alive.any():
            break
        S = M2[c[None, :], QT]
        eq = (c[None, :] == QT).astype(np.int64)
        s = H[1:] + S                                            # the previous column's H[k + 1]
        pos = s > 0
        cell = np.where(pos, s, 0)
        m = np.where(pos, AM[1:] + eq, 0)
        ln = np.where(pos, AL[1:] + 1, 0)
        En = np.maximum(E[:-1] + ext_gap, H[:-1] + open_gap)
        use_e = En > cell
        cell = np.where(use_e, En, cell)
        m = np.where(use_e, AM[:-1], m)
        ln = np.where(use_e, AL[:-1] + 1, ln)
        Hn = np.zeros_like(H)
        AMn = np.zeros_like(AM)
        ALn = np.zeros_like(AL)
        F = np.zeros(n, dtype=np.int64)
        for k in range(L - 1, -1, -1):
            F = np.maximum(F + ext_gap, Hn[k + 1] + open_gap)    # this column's H[k + 1]
            use_f = F > cell[k]
            Hn[k] = np.where(use_f, F, cell[k])
            AMn[k] = np.where(use_f, AMn[k + 1], m[k])
            ALn[k] = np.where(use_f, ALn[k + 1] + 1, ln[k])
        colmax = Hn[:L].max(axis=0)
        kstar = L - 1 - np.argmax(Hn[:L][::-1], axis=0)          # rows run downwards: the highest row first
        for w, bst in zip(widths, best):
            upd = alive & (j < w) & (colmax > bst[0])
            bst[0] = np.where(upd, colmax, bst[0])
            bst[1] = np.where(upd, j, bst[1])
            bst[2] = np.where(upd, AMn[kstar, cols], bst[2])
            bst[3] = np.where(upd, ALn[kstar, cols], bst[3])
        H, AM, AL = Hn, AMn, ALn
        E[:-1] = En
    out = tuple((end - bst[1], bst[3], bst[2]) for bst in best)
    return out if isinstance(base, tuple) else out[0]


# ---------------------------------------------------------------- matrices
def diag_matrix(m: int) -> np.ndarray:
    """+m on the diagonal of codes 0..24, seeded off-diagonal values in
    [-m, m // 4] that are not symmetric, a non-zero X row and column, -m at
    [0][1] (and not at [1][0]). max|M| = m, so an exact copy scores L * m."""
    r = random.Random(1000 + m)
    M = np.zeros((32, 32), dtype=np.int32)
    for a in range(25):
        for b in range(25):
            M[a, b] = m if a == b else r.randint(-m, m // 4)
    for a in range(25):
        if a != X:
            if M[X, a] == 0:
                M[X, a] = -1
            if M[a, X] == 0:
                M[a, X] = -1
    M[0, 1] = -m
    M[1, 0] = m // 4
    assert not np.array_equal(M, M.T) and int(np.abs(M).max()) == m
    return np.ascontiguousarray(M.reshape(-1))


def negative_matrix() -> np.ndarray:
    r = random.Random(77)
    M = np.zeros((32, 32), dtype=np.int32)
    for a in range(25):
        for b in range(25):
            M[a, b] = -r.randint(1, 4)
    return np.ascontiguousarray(M.reshape(-1))


def codes_matrix() -> np.ndarray:
    """diag(11) with seeded non-zero rows for the DB codes 26..31 (max|M| stays 11)."""
    r = random.Random(2631)
    M = diag_matrix(11).reshape(32, 32).copy()
    for c in range(26, 32):
        for q in range(25):
            M[c, q] = r.choice([v for v in range(-11, 12) if v])
    return np.ascontiguousarray(M.reshape(-1))


def zero_matrix() -> np.ndarray:
    return np.zeros(32 * 32, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def matrix(name: str) -> np.ndarray:
    """blosum62 | pam250 | neg | zero | diag<m>"""
    if name == "blosum62":
        return tx.blosum62()
    if name == "pam250":
        return tx.pam250()
    if name == "neg":
        return negative_matrix()
    if name == "zero":
        return zero_matrix()
    if name == "diag11x":
        return codes_matrix()
    assert name.startswith("diag"), name
    return diag_matrix(int(name[4:]))


# ---------------------------------------------------------------- the fixture
MOTIF = "MWCHW"


def _subjects():
    """The DB of every width, about 4000 residues: a subject flush at the DB's
    start; subjects of 5, 12 and 40 residues in a row and eight more of 5-9, so
    that one score window meets 1, 2 and many ENDs; a 60-residue segment twice
    within 120 columns (ties for the end column's >= and the start's >); random
    subjects of 150-300; the motif planted 30 times; a subject flush at the end."""
    r = random.Random(20)
    rnd = lambda n: "".join(r.choice(AA) for _ in range(n))  # noqa: E731
    subj = [("first", rnd(140)), ("t5", rnd(5)), ("t12", rnd(12)), ("t40", rnd(40))]
    subj += [(f"tiny{i}", rnd(r.randint(5, 9))) for i in range(8)]
    seg = rnd(60)
    subj.append(("rep", rnd(70) + seg + seg + rnd(70)))
    for i in range(12):
        s = list(rnd(r.randint(150, 300)))
        for p in (20, 75, 130)[: 3 if i < 6 else 2]:
            s[p:p + len(MOTIF)] = MOTIF
        subj.append((f"s{i}", "".join(s)))
    subj.append(("last", rnd(140)))
    return subj


def _mutate(r, s, rate):
    return "".join(r.choice(AA) if r.random() < rate else ch for ch in s)


def _kmer_positions(subj):
    occ = {}
    for _, s in subj:
        for p in range(len(s) - 2):
            occ.setdefault(s[p:p + 3], 0)
            occ[s[p:p + 3]] += 1
    return occ


def queries(L: int):
    """[(class, sequence)] for width L, about 40 queries; sequences longer than
    L are cut by the formatter, shorter ones are X-padded."""
    subj = dict(_subjects())
    names = [n for n, _ in _subjects()]
    r = random.Random(100 + L)
    big = [n for n in names if len(subj[n]) >= 140]
    out = []

    def copy(name, off, n=L):
        return subj[name][off:off + n]

    # exact copies: the DB's first and last residues, the repeat, random places
    out.append(("exact_first", copy("first", 0)))
    out.append(("exact_last", subj["last"][-L:]))
    out.append(("exact_rep", copy("rep", 70)))
    out.append(("exact_rep", copy("rep", 70 + max(0, 60 - L))))
    for _ in range(4):
        nme = r.choice(big)
        out.append(("exact", copy(nme, r.randint(0, len(subj[nme]) - L))))
    # copies that span a subject boundary (the query has no END: the two sides are joined)
    h = (L + 1) // 2
    tinies = subj["t5"] + subj["t12"] + subj["t40"] + "".join(subj[f"tiny{i}"] for i in range(8))
    out.append(("boundary", subj["first"][-h:] + tinies[:L - h]))
    out.append(("boundary", subj["s10"][-h:] + subj["s11"][:L - h]))
    out.append(("boundary", subj["s11"][-h:] + subj["last"][:L - h]))
    out.append(("boundary", (tinies + subj["rep"])[:L]))
    out.append(("boundary", ("".join(subj[f"tiny{i}"] for i in range(8)) + subj["rep"])[:L]))  # 5-9 residues per subject
    # one insertion and one deletion of 1, 3 and 10 residues
    for nres in (1, 3, 10):
        for kind in ("ins", "del"):
            nme = r.choice(big)
            off = r.randint(0, len(subj[nme]) - (L + 10))
            s = list(copy(nme, off, L + 10))
            p = max(1, L // 2)
            if kind == "ins":
                s[p:p] = [r.choice(AA) for _ in range(nres)]
            else:
                del s[p:p + nres]
            out.append((f"{kind}{nres}", "".join(s[:L])))
    # mutated copies
    for rate in (0.1, 0.2, 0.3, 0.1, 0.2, 0.3):
        nme = r.choice(big)
        out.append(("mut", _mutate(r, copy(nme, r.randint(0, len(subj[nme]) - L)), rate)))
    # shorter than L, down to the seed span (X padding)
    for n in sorted({SEED_K, SEED_K + 1, max(SEED_K, L // 2), max(SEED_K, L - 1)}):
        if n < L:
            nme = r.choice(big)
            out.append(("short", copy(nme, r.randint(0, len(subj[nme]) - n), n)))
    # 1, 2 and 3 candidates: a 3-mer that occurs so many times in the DB; >= 24: the planted motif
    if L >= SEED_K:
        occ = _kmer_positions(_subjects())
        for want in (1, 2, 3):
            # (not from the DB's first 32 columns: a hit in diagonal bin 1 also makes bin 0 a candidate)
            kmers = sorted(k for k, v in occ.items() if v == want and not set(k) & set(MOTIF)
                           and k not in subj["first"][:40])
            out.append((f"cands{want}", r.choice(kmers)))
        for s in (MOTIF[:3], MOTIF[:4], MOTIF, MOTIF[1:], MOTIF[2:]):
            out.append(("cands24", s[:L]))
    return out


def write_fixture(d: str, L: int) -> None:
    with open(os.path.join(d, "db.fa"), "w") as f:
        f.write("".join(tx._fasta(n, s) for n, s in _subjects()))
    with open(os.path.join(d, "q.fa"), "w") as f:
        f.write("".join(tx._fasta(f"q{i}_{c}", s) for i, (c, s) in enumerate(queries(L))))


def build_fixture(root: str, L: int) -> str:
    d = os.path.join(root, f"dp_L{L}")
    stamp = os.path.join(d, ".done")
    if not os.path.exists(stamp):
        os.makedirs(d, exist_ok=True)
        write_fixture(d, L)
        subprocess.run([cases.GHOSTM, "db", "-i", f"{d}/db.fa", "-o", f"{d}/db", "-k", str(SEED_K)], check=True,
                       capture_output=True)
        subprocess.run([cases.GHOSTM, "qry", "-i", f"{d}/q.fa", "-o", f"{d}/q", "-l", str(L)], check=True,
                       capture_output=True)
        open(stamp, "w").close()
    return d


class Fixture:
    """The formatted chunk of one width, with its query classes."""

    def __init__(self, root: str, L: int):
        self.d = build_fixture(root, L)
        self.nq, self.L, self.qseq, self.db, self.pos = tx.load_chunk(self.d)
        self.seed, self.kc, self.ipos = tx.load_index(self.d)
        self.classes = [c for c, _ in queries(L)]
        assert self.L == L and self.nq == len(self.classes), (self.L, self.nq, len(self.classes))
        self._cand = None
        self._codes = None

    def oracle(self, opts=(), tag="default"):
        """The oracle's (.cand, .tb) dumps for `aln -t 1 opts`: u32 (qid, start,
        score, end) per candidate and (qid, end, start, len, match) per traceback."""
        dump_dir = os.path.join(self.d, "dump_" + tag)
        os.makedirs(dump_dir, exist_ok=True)
        prefix = os.path.join(dump_dir, "dump")
        if not os.path.exists(prefix + ".ok"):
            for suffix in (".tb", ".cand"):
                if os.path.exists(prefix + suffix):
                    os.remove(prefix + suffix)
            cases.run_aln(cases.ORACLE, self.d, ["-y", "1", "-t", str(THRESHOLD)] + list(opts),
                          {"GHOSTM_ORACLE_DUMP": prefix}, os.path.join(dump_dir, "o"))
            open(prefix + ".ok", "w").close()
        cand = np.fromfile(prefix + ".cand", dtype="<u4").reshape(-1, 4)
        tb = np.fromfile(prefix + ".tb", dtype="<u4").reshape(-1, 5) if os.path.exists(prefix + ".tb") else \
            np.zeros((0, 5), dtype=np.uint32)
        return cand, tb

    def db_codes(self):
        """The DB with 24 residues patched to the codes 26..31 after indexing (no
        formatter writes them; K1 reads the index alone, so the candidates stay):
        four in each of the first, the repeat, the last and three other subjects."""
        if self._codes is None:
            db = self.db.copy()
            starts = [int(p) for p in self.pos]
            k = 0
            for s in (0, 12, 13, 16, 20, len(starts) - 1):
                for off in (6, 41, 77, 118):
                    assert db[starts[s] + off] < END
                    db[starts[s] + off] = 26 + k % 6
                    k += 1
            self._codes = db
        return self._codes

    def candidates(self):
        """(qid, start) of the oracle's candidates (they do not depend on the matrix)."""
        if self._cand is None:
            cand, _ = self.oracle()
            self._cand = (np.ascontiguousarray(cand[:, 0]), np.ascontiguousarray(cand[:, 1]))
        return self._cand


_FIXTURES = {}
_MODEL = {}


def fixture(root: str, L: int) -> Fixture:
    if (root, L) not in _FIXTURES:
        _FIXTURES[(root, L)] = Fixture(root, L)
    return _FIXTURES[(root, L)]


def score_base(L: int, extend: int = 2, region: int = 16) -> int:
    return L + 2 * extend + 2 * region


def trace_base(L: int, extend: int = 2, region: int = 16) -> int:
    return L + 2 * extend * 2 * region


def model_scores(root: str, L: int, mname: str, gaps=(-11, -1), codes=False):
    """The model's (score, end) of every candidate of the width's fixture
    (codes: on Fixture.db_codes); cached."""
    key = ("score", root, L, mname, gaps) + (("codes",) if codes else ())
    if key not in _MODEL:
        fx = fixture(root, L)
        qid, start = fx.candidates()
        db = fx.db_codes() if codes else fx.db
        _MODEL[key] = score_model(fx.qseq, L, db, matrix(mname), qid, start, score_base(L), 2, gaps[0], gaps[1])
    return _MODEL[key]


def hand_hits(fx: Fixture):
    """Hand-placed hits beside the candidates' ends: ends below every window
    (end < base), on the DB's last residue, and three hits of one query so
    that some query has an odd number of hits."""
    last = len(fx.db) - 1
    while fx.db[last] == END:
        last -= 1
    first = 0
    while fx.db[first] == END:
        first += 1
    q_first = fx.classes.index("exact_first")
    q_last = fx.classes.index("exact_last")
    hits = [(q_first, first), (q_first, first + fx.L - 1), (q_first, first + min(fx.L, 139)), (q_last, last),
            (q_last, last - 1), (q_last, last - 2), (q_last, last - 3)]
    return (np.array([h[0] for h in hits], dtype=np.uint32), np.array([h[1] for h in hits], dtype=np.uint32))


def model_hits(root: str, L: int, mname: str, gaps=(-11, -1), codes=False):
    """(qid, end) to trace: every candidate's model end under (matrix, gaps)
    where the width seeds, plus the hand-placed hits."""
    fx = fixture(root, L)
    hq, he = hand_hits(fx)
    if L >= SEED_K:
        qid, _ = fx.candidates()
        _, end = model_scores(root, L, mname, gaps, codes)
        hq = np.concatenate([qid, hq]).astype(np.uint32)
        he = np.concatenate([end.astype(np.uint32), he]).astype(np.uint32)
    return np.ascontiguousarray(hq), np.ascontiguousarray(he)


def model_traces(root: str, L: int, mname: str, gaps=(-11, -1), base=None, codes=False):
    """((qid, end), (start, len, match)) of model_hits under the window `base`
    (L + 128 by default); cached, and computed together with the wide window's
    (L + 512)."""
    base = trace_base(L) if base is None else base
    tail = ("codes",) if codes else ()
    key = ("trace", root, L, mname, gaps, base) + tail
    if key not in _MODEL:
        fx = fixture(root, L)
        hq, he = model_hits(root, L, mname, gaps, codes)
        # neighbouring candidates often end in the same column: the DP of a (qid, end) pair runs once
        pairs, inv = np.unique(np.stack([hq, he], axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        bases = tuple(sorted({base, trace_base(L), trace_base(L, region=64)}))
        outs = trace_model(fx.qseq, L, fx.db_codes() if codes else fx.db, matrix(mname), pairs[:, 0], pairs[:, 1],
                           bases, gaps[0], gaps[1])
        for b, out in zip(bases, outs):
            _MODEL[("trace", root, L, mname, gaps, b) + tail] = ((hq, he), tuple(a[inv] for a in out))
    return _MODEL[key]


def save_models(root: str) -> str:
    """The cached model results as a file a child process reads (load_models)."""
    import pickle

    path = os.path.join(root, "dp_models.pkl")
    with open(path, "wb") as f:
        pickle.dump(_MODEL, f)
    return path


def load_models(root: str) -> None:
    import pickle

    with open(os.path.join(root, "dp_models.pkl"), "rb") as f:
        _MODEL.update(pickle.load(f))


# ---------------------------------------------------------------- the device side
# every forced form of the two launches (GHOSTM_K2_PAIR_S acts on the pair kernel)
K2_FORMS = [{}] + [{"GHOSTM_K2": v} for v in ("int32", "int16", "f16plain", "f16frame", "swar16", "unit", "pair",
                                              "sparse")] + \
    [{"GHOSTM_K2_LEVELS": "0"}, {"GHOSTM_K2_TASKS": "paired"}, {"GHOSTM_K2_TASKS": "consecutive"},
     {"GHOSTM_K2_PAIR_S": "8"}, {"GHOSTM_K2_PAIR_S": "16"}, {"GHOSTM_K2": "pair", "GHOSTM_K2_PAIR_S": "8"},
     {"GHOSTM_K2": "pair", "GHOSTM_K2_PAIR_S": "16"}]
K3_FORMS = [{}, {"GHOSTM_K3": "int32"}] + [{"GHOSTM_K3_SCAN": v} for v in ("0", "int16", "f16plain", "f16frame",
                                                                           "priv")] + \
    [{"GHOSTM_K3_STRIPS": "0"}, {"GHOSTM_K3_KEYFRAME": "0"}, {"GHOSTM_K3_SCAN_S": "16"}]
FORCING = sorted({k for f in K2_FORMS + K3_FORMS for k in f})


class forced:
    """The environment of one forced form, and of no other, for the calls inside."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in FORCING}
        for k in FORCING:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Stage:
    """One fixture resident on the device through the reference plugin ABI:
    InitGpu, SetOptionGpu, SetQueryGpu, SetDbGpu; then K1 once, K2 and K3 with
    any matrix, gaps and window."""

    def __init__(self, fx: Fixture, db=None):
        import ctypes

        from ghostm_amd import native

        self.ct, self.native, self.lib, self.fx = ctypes, native, native.load(), fx
        self.db = np.ascontiguousarray(fx.db if db is None else db)
        assert self.lib.InitGpu() == 0
        self.set_matrix(matrix("blosum62"))
        assert self.lib.SetQueryGpu(tx._p(fx.qseq, ctypes.c_uint8), fx.nq, fx.L) == 0, native.last_error()
        assert self.lib.SetDbGpu(tx._p(self.db, ctypes.c_uint8), len(self.db), tx._p(fx.kc), len(fx.kc),
                                 tx._p(fx.ipos), len(fx.ipos)) == 0, native.last_error()
        self.n = None

    def set_matrix(self, M):
        M = np.ascontiguousarray(M, dtype=np.int32)
        assert self.lib.SetOptionGpu(1 << 27, M.ctypes.data_as(self.ct.POINTER(self.ct.c_int)), 0) == 0, \
            self.native.last_error()

    def search(self, cap: int):
        """K1: (qid, start) of every candidate (cap: room for the starts)."""
        fx = self.fx
        acl = np.zeros(fx.nq + 1, dtype=np.uint32)
        starts = np.zeros(cap + 64, dtype=np.uint32)
        counts = np.zeros(fx.nq, dtype=np.uint32)
        assert self.lib.CountCandidatesGpu(fx.L, fx.nq, fx.seed, THRESHOLD, 2, 4, tx._p(counts)) == 0
        assert int(counts.sum()) <= cap, (int(counts.sum()), cap)  # nothing is written past the buffer
        qc = self.lib.SearchNextGpu(fx.L, fx.nq, fx.seed, THRESHOLD, 2, 4, 1 << 27, 0, tx._p(acl), tx._p(starts))
        assert qc == fx.nq, self.native.last_error()
        self.n = int(acl[qc])
        assert np.array_equal(np.diff(acl[:qc + 1]), counts)
        qid = np.repeat(np.arange(fx.nq, dtype=np.uint32), np.diff(acl[:qc + 1]))
        return qid, starts[:self.n].copy()

    def score(self, base, gaps, extend=2):
        """K2 on the candidates of the last search: (score, end)."""
        scores = np.full(self.n, 0xDEAD, dtype=np.uint32)
        ends = np.full(self.n, 0xDEAD, dtype=np.uint32)
        self.lib.CalculateScoreGpu(len(self.db), self.fx.L, self.n, tx._p(scores), tx._p(ends), base, extend,
                                   gaps[0], gaps[1])
        assert self.native.last_error() == "", self.native.last_error()
        return scores, ends

    def trace(self, qid, end, base, gaps):
        """K3: (start, len, match) of the hits (qid, end)."""
        n = len(qid)
        out = [np.full(n, 0xDEAD, dtype=np.uint32) for _ in range(3)]
        ident = np.zeros(n, dtype=np.float32)
        rc = self.lib.TraceBackGpu(n, tx._p(qid), tx._p(end), self.fx.L, base, gaps[0], gaps[1], tx._p(out[0]),
                                   tx._p(out[1]), tx._p(out[2]), ident.ctypes.data_as(self.ct.POINTER(self.ct.c_float)))
        assert rc == 0, self.native.last_error()
        return out

    def counters(self) -> dict:
        st = self.native.GhostmStats()
        assert self.lib.GhostmStageStats(self.ct.byref(st), self.ct.sizeof(st)) == self.ct.sizeof(st)
        return st.as_dict()

    def close(self):
        assert self.lib.FreeGpu() == 0


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} differ, first at {bad[:5].tolist()}: "
                             f"got {got[bad[:5]].tolist()}, model {want[bad[:5]].tolist()}")


def check_k2(st: Stage, root, L, mname, gaps=(-11, -1), forms=K2_FORMS, codes=False):
    """CalculateScoreGpu's score and end of every candidate equal the model's,
    in every form. Returns the counters' increase over the default-form launch."""
    want_score, want_end = model_scores(root, L, mname, gaps, codes)
    st.set_matrix(matrix(mname))
    delta = None
    for env in forms:
        with forced(env):
            before = st.counters()
            score, end = st.score(score_base(L), gaps)
            after = st.counters()
        if not env:
            delta = {k: after[k] - before[k] for k in after}
        _same(score, want_score, f"K2 score L={L} {mname} gaps={gaps} {env}")
        _same(end, want_end, f"K2 end L={L} {mname} gaps={gaps} {env}")
    return delta


def check_k3(st: Stage, root, L, mname, gaps=(-11, -1), base=None, forms=K3_FORMS, codes=False):
    """TraceBackGpu's (start, len, match) of model_hits equal the model's, in
    every form. Returns the counters' increase over the default-form launch."""
    base = trace_base(L) if base is None else base
    (qid, end), want = model_traces(root, L, mname, gaps, base, codes)
    st.set_matrix(matrix(mname))
    delta = None
    for env in forms:
        with forced(env):
            before = st.counters()
            got = st.trace(qid, end, base, gaps)
            after = st.counters()
        if not env:
            delta = {k: after[k] - before[k] for k in after}
        for g, w, what in zip(got, want, ("start", "len", "match")):
            _same(g, w, f"K3 {what} L={L} {mname} gaps={gaps} base={base} {env}")
    return delta


WIDTH_MATRICES = ["blosum62", "pam250", "diag11"]


def layout_sweep(root, widths, forms2=({},), forms3=({},)):
    """Every width with BLOSUM62, PAM250 and diag(11): K2 (where the width seeds)
    and K3 at both windows against the model. Returns the candidates and hits compared."""
    ncand = nhits = 0
    for L in widths:
        fx = fixture(root, L)
        st = Stage(fx)
        if L >= SEED_K:
            want_qid, want_start = fx.candidates()
            qid, start = st.search(len(want_qid))
            _same(qid, want_qid, f"K1 qid L={L}")
            _same(start, want_start, f"K1 start L={L}")
            ncand += len(qid)
        for mname in WIDTH_MATRICES:
            if L >= SEED_K:
                check_k2(st, root, L, mname, forms=forms2)
            for base in (trace_base(L), trace_base(L, region=64)):
                check_k3(st, root, L, mname, base=base, forms=forms3)
                nhits += len(model_hits(root, L, mname)[0])
        st.close()
    return ncand, nhits
