"""The adapter stage's Python model and case sets (GhostmAdapterTrimHost,
AdapterTrimGpu; the rule is above GhostmAdapterTrimHost in include/ghostm_hip.h).

The model is the issue's, letter by letter. Adapter rule: a start p, L = min(m,
n - p), mm(p) the mismatches over L (an adapter N matches everything, a read
byte that is none of ACGT after upper-casing nothing else), p accepted when L >=
min_overlap and mm * 100 <= err_pct * L, adapter_at the smallest accepted p or
n. Pair rule: f in pair_overlap..min(n1, n2), pm(f) the i < f where R1[i] is not
the complement of R2[f - 1 - i], f accepted when pm * 100 <= err_pct * f,
pair_len the greatest accepted f or 0; mates of over 1024 letters are skipped.
kept = min(adapter_at, pair_len or n).

The sets: reads of the lengths around the kernel's 64-start groups with the
adapter planted at the starts the issue names, random reads and random pairs
with read-through, all laid at odd byte offsets in one buffer with gap bytes
between them that spell the adapter's first letters (a kernel that read a byte
behind its read would find an adapter there), and the named cases, each with
the result it must give written down beside the model's."""
import functools
import random

import numpy as np

OUT_DTYPE = np.dtype([("kept", "<u4"), ("adapter_at", "<u4"), ("pair_len", "<u4"),
                      ("adapter_mismatches", "<u2"), ("pair_mismatches", "<u2")])
PAIR_LETTERS_MAX = 1024
TRUSEQ = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"   # 33 letters
TRUSEQ2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"  # mate 2's
SUM_KEYS = ("reads", "letters", "cut_reads", "cut_letters", "adapter_found", "pair_found", "pair_skipped", "emptied")
COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def P(a1=b"", a2=b"", mo=5, err=10, po=0):
    """the stage's parameters in the order of adapter_trim's arguments"""
    return (bytes(a1), bytes(a2), mo, err, po)


# ------------------------------------------------------------------ the model
def up(b):
    return b - 32 if ord("a") <= b <= ord("z") else b


_READ_CODE = np.full(256, 4, dtype=np.uint8)     # a read byte: A C G T = 0..3 in either case, everything else 4
_ADAPTER_CODE = np.full(256, 9, dtype=np.uint8)  # an adapter byte: likewise, N = 8
for _k, _c in enumerate(b"ACGT"):
    _READ_CODE[_c] = _READ_CODE[_c + 32] = _ADAPTER_CODE[_c] = _ADAPTER_CODE[_c + 32] = _k
_ADAPTER_CODE[ord("N")] = _ADAPTER_CODE[ord("n")] = 8


def codes(read):
    return _READ_CODE[np.frombuffer(bytes(read), dtype=np.uint8)]


def adapter_at(read, adapter, mo, err):
    """(adapter_at, its mismatches)"""
    n, m = len(read), len(adapter)
    if m == 0:
        return n, 0
    rd, ad = codes(read), _ADAPTER_CODE[np.frombuffer(bytes(adapter), dtype=np.uint8)]
    assert (ad != 9).all()
    for p in range(n):
        L = min(m, n - p)
        mm = int(((rd[p:p + L] != ad[:L]) & (ad[:L] != 8)).sum())  # a read's 4 equals no adapter letter
        if L >= mo and mm * 100 <= err * L:
            return p, mm
    return n, 0


def pair_len(r1, r2, po, err):
    """(pair_len, its mismatches, skipped)"""
    n1, n2 = len(r1), len(r2)
    if po == 0:
        return 0, 0, False
    if n1 > PAIR_LETTERS_MAX or n2 > PAIR_LETTERS_MAX:
        return 0, 0, True
    c1, c2 = codes(r1), codes(r2)
    comp2 = np.where(c2 < 4, 3 - c2, 5).astype(np.uint8)  # the complement; 5 equals nothing on mate 1
    for f in range(min(n1, n2), po - 1, -1):
        pm = int((c1[:f] != comp2[:f][::-1]).sum())  # R1[i] against the complement of R2[f - 1 - i]
        if pm * 100 <= err * f:
            return f, pm, False
    return 0, 0, False


def model_reads(reads, params):
    """reads: a list of bytes -> (OUT_DTYPE records, the counters' sums)"""
    a1, a2, mo, err, po = params
    out = np.zeros(len(reads), dtype=OUT_DTYPE)
    sums = dict.fromkeys(SUM_KEYS, 0)
    on = bool(a1 or a2 or po)
    if po:
        assert len(reads) % 2 == 0
    for r, read in enumerate(reads):
        n = len(read)
        if not on:
            out[r] = (n, n, 0, 0, 0)
            continue
        f = pm = 0
        if po:
            e = r & ~1
            f, pm, skipped = pair_len(reads[e], reads[e + 1], po, err) if r == e else (int(out[e]["pair_len"]), int(out[e]["pair_mismatches"]), False)
            if r == e:
                sums["pair_found"] += f > 0
                sums["pair_skipped"] += skipped
        at, mm = adapter_at(read, a2 if (r & 1) and a2 else a1, mo, err)
        kept = min(at, f if f else n)
        out[r] = (kept, at, f, mm, pm)
        sums["reads"] += 1
        sums["letters"] += n
        sums["cut_reads"] += kept < n
        sums["cut_letters"] += n - kept
        sums["adapter_found"] += at < n
        sums["emptied"] += n > 0 and kept == 0
    return out, sums


# ------------------------------------------------------------------ laying out
def lay_out(reads, filler=b"#", seed=1):
    """reads: a list of bytes -> (letters, offsets, lengths): every read at an odd offset behind 1..4 gap bytes, the
    gap bytes those of filler from its start, and gap bytes at the end."""
    rnd = random.Random(seed)
    letters, offs, lens = bytearray(), [], []
    filler = bytes(filler) or b"#"
    fill = lambda k: (filler * 5)[:k]  # noqa: E731
    for ls in reads:
        gap = rnd.randint(1, 4)
        if (len(letters) + gap) % 2 == 0:
            gap += 1
        letters += fill(gap)
        offs.append(len(letters))
        lens.append(len(ls))
        letters += ls
    letters += fill(5)
    return bytes(letters), np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32)


def rand_letters(rnd, n, alphabet=b"ACGT"):
    return bytes(rnd.choice(alphabet) for _ in range(n))


def revcomp(s):
    return bytes(COMP[b] for b in reversed(s))


def with_errors(rnd, s, k, avoid=()):
    """s with k letters replaced by another of ACGT, at distinct places outside avoid"""
    s = bytearray(s)
    for i in rnd.sample([i for i in range(len(s)) if i not in avoid], k):
        s[i] = rnd.choice([b for b in b"ACGT" if b != up(s[i])])
    return bytes(s)


def plant(background, p, adapter):
    """the background with the adapter over its letters from p on, as far as its length allows"""
    n = len(background)
    return (background[:p] + adapter + background[p + len(adapter):])[:n] if p < n else background


# ------------------------------------------------------------------ the adapter sets
M_VALUES = (1, 33, 63, 64)
FIXED_LENGTHS = lambda mo: [0, 1, mo - 1, mo, 63, 64, 65, 127, 128, 129]  # noqa: E731


def adapter_of(m, seed=0):
    rnd = random.Random(100 + m + seed)
    return (TRUSEQ + rand_letters(rnd, 64))[:m] if m >= 33 else rand_letters(rnd, m)


def fixed_set(m, mo, seed=0):
    """The fixed lengths, each with the adapter planted at 0, 63, 64, n - mo and n - mo + 1 (where inside the read) in
    a random background, and unplanted."""
    rnd = random.Random(7 * m + mo + seed)
    adapter = adapter_of(m)
    reads = []
    for n in FIXED_LENGTHS(mo):
        reads.append(rand_letters(rnd, n))
        for p in (0, 63, 64, n - mo, n - mo + 1):
            if 0 <= p < n:
                reads.append(plant(rand_letters(rnd, n), p, adapter))
    return reads, adapter


def random_set(m, mo, err, seed=0):
    """About 250 random reads of 20..300 letters: a third untouched, the others with the adapter planted, with up
    to three wrong letters, some with N's and lower case."""
    rnd = random.Random(1000 * seed + 31 * m + 7 * mo + err)
    adapter = adapter_of(m)
    reads = []
    for k in range(250):
        n = rnd.randint(20, 300)
        read = rand_letters(rnd, n, b"ACGTACGTACGTN" if k % 5 == 0 else b"ACGT")
        if k % 3:
            p = rnd.randint(0, n - 1)
            read = plant(read, p, with_errors(rnd, adapter, min(rnd.randint(0, 3), m)))
        if k % 7 == 0:
            read = read.lower()
        reads.append(read)
    return reads, adapter


ADAPTER_SETS = [(m, mo, err) for m in M_VALUES for mo, err in ((5, 10), (1, 0), (3, 20))] + [(64, 64, 50), (33, 8, 10)]


# ------------------------------------------------------------------ the pair sets
def read_through(rnd, f, n1, n2, tail1=TRUSEQ, tail2=TRUSEQ2, errors=0):
    """Mates of n1 and n2 letters of a fragment of f letters: each is the fragment's strand, then its adapter, then
    random letters."""
    frag = rand_letters(rnd, f)
    r1 = (frag + tail1 + rand_letters(rnd, n1))[:n1]
    r2 = (revcomp(frag) + tail2 + rand_letters(rnd, n2))[:n2]
    if errors:
        r1 = with_errors(rnd, r1[:f], errors) + r1[f:]
    return r1, r2


def random_pairs(po, err, seed=0, count=120):
    """Random pairs of 30..300 letters: a third without overlap, the others read through at a fragment of 1..min
    letters with up to two wrong letters; every tenth pair with N's."""
    rnd = random.Random(500 * seed + 3 * po + err)
    reads = []
    for k in range(count):
        n1, n2 = rnd.randint(30, 300), rnd.randint(30, 300)
        if k % 3 == 0:
            r1, r2 = rand_letters(rnd, n1), rand_letters(rnd, n2)
        else:
            r1, r2 = read_through(rnd, rnd.randint(1, min(n1, n2)), n1, n2, errors=0)
            r1 = with_errors(rnd, r1, rnd.randint(0, 2))
        if k % 10 == 0:
            r1 = r1[:7] + b"N" + r1[8:]
            r2 = r2[:11] + b"n" + r2[12:]
        if k % 11 == 0:
            r2 = r2.lower()
        reads += [r1, r2]
    return reads


PAIR_SETS = [(20, 10), (8, 10), (1, 0), (12, 50)]


# ------------------------------------------------------------------ the named cases
@functools.lru_cache(maxsize=None)
def named_cases():
    """name -> (reads, params, want): want is a list with one entry per read, (kept, adapter_at, pair_len) or None
    where only the model speaks. check_sets() asserts that the model gives what is written down."""
    rnd = random.Random(77)
    cases = {}
    AD = b"ACGGACGCAGGACCAGCAGGCACGACAGGCAGA"  # 33 letters without T: a background of T's matches it nowhere
    assert len(AD) == 33 and b"T" not in AD
    T = lambda k: b"T" * k  # noqa: E731
    p510 = P(AD, b"", 5, 10, 0)

    # found at n - min_overlap, not found one further
    cases["tail_of_min_overlap_found"] = ([T(95) + AD[:5]], p510, [(95, 95, 0)])
    cases["tail_below_min_overlap_not_found"] = ([T(96) + AD[:4]], p510, [(100, 100, 0)])
    # the thresholds: L = 10 and 19 take one mismatch and not two, L = 20 takes two and not three
    for L, ok, over in ((10, 1, 2), (19, 1, 2), (20, 2, 3)):
        for k in (ok, over):
            tail = bytearray(AD[:L])
            for i in range(k):
                tail[2 + 3 * i] = ord("T")
            want = (70, 70, 0) if k == ok else (70 + L, 70 + L, 0)
            cases[f"threshold_L{L}_mm{k}"] = ([T(70) + bytes(tail)], p510, [want])
    tail = bytearray(AD)
    tail[17] = ord("T")
    cases["err_pct_0_exact"] = ([T(10) + AD + T(20)], P(AD, b"", 5, 0, 0), [(10, 10, 0)])
    cases["err_pct_0_one_wrong"] = ([T(10) + bytes(tail) + T(20)], P(AD, b"", 5, 0, 0), [(63, 63, 0)])
    # two accepted starts: the leftmost wins
    cases["two_starts_in_two_groups"] = ([T(10) + AD + T(57) + AD + T(7)], p510, [(10, 10, 0)])
    cases["two_starts_in_one_group"] = ([T(10) + AD + T(2) + AD + T(7)], p510, [(10, 10, 0)])
    cases["start_at_lane_63_and_64"] = ([T(63) + AD + T(4), T(64) + AD + T(4)], p510, [(63, 63, 0), (64, 64, 0)])
    # letters: an adapter N matches anything, a read N nothing but it; lower case is upper-cased
    ADN = AD[:4] + b"NN" + AD[6:20] + b"n" + AD[21:]
    cases["adapter_N_is_a_wildcard"] = ([T(30) + AD[:4] + b"TN" + AD[6:20] + b"#" + AD[21:] + T(5)],
                                        P(ADN, b"", 5, 0, 0), [(30, 30, 0)])
    cases["read_N_is_a_mismatch"] = ([T(30) + AD[:8] + b"N" + AD[9:] + T(5)], P(AD, b"", 5, 0, 0), [(68, 68, 0)])
    cases["read_N_within_the_budget"] = ([T(30) + AD[:8] + b"N" + AD[9:] + T(5)], p510, [(30, 30, 0)])
    cases["lowercase_read"] = ([T(30).lower() + AD.lower() + T(5)], p510, [(30, 30, 0)])
    cases["lowercase_adapter"] = ([T(30) + AD + T(5)], P(AD.lower(), b"", 5, 10, 0), [(30, 30, 0)])
    # adapter2 is for the odd records only
    AD2 = b"CAGCAGGAACCGACAGGAACGCCAGAGGACGAC"
    assert len(AD2) == 33 and b"T" not in AD2
    four = [T(40) + AD + T(3), T(40) + AD + T(3), T(40) + AD2 + T(3), T(40) + AD2 + T(3)]
    cases["adapter2_on_odd_records"] = (four, P(AD, AD2, 5, 10, 0), [(40, 40, 0), (76, 76, 0), (76, 76, 0), (40, 40, 0)])
    cases["adapter2_alone"] = (four, P(b"", AD2, 5, 10, 0), [(76, 76, 0), (76, 76, 0), (76, 76, 0), (40, 40, 0)])
    cases["adapter1_for_all_without_adapter2"] = (four, p510, [(40, 40, 0), (40, 40, 0), (76, 76, 0), (76, 76, 0)])
    # a one-letter adapter at min_overlap 1: the first such letter
    cases["one_letter_adapter"] = ([T(64) + b"G" + T(10), T(70)], P(b"G", b"", 1, 0, 0), [(64, 64, 0), (70, 70, 0)])

    # ---- the pair rule; tails of T on mate 1 and of A... no: both tails of T, whose complement A is in neither
    def mates(f, n1, n2, frag=None):
        frag = frag if frag is not None else rand_letters(rnd, f, b"ACG")
        return [(frag + T(n1))[:n1], (revcomp(frag) + T(n2))[:n2]]
    pp = lambda po, err=10: P(b"", b"", 5, err, po)  # noqa: E731
    cases["pair_f_is_pair_overlap"] = (mates(20, 100, 100), pp(20), [(20, 100, 20)] * 2)
    cases["pair_f_below_pair_overlap"] = (mates(19, 100, 100), pp(20), [(100, 100, 0)] * 2)
    cases["pair_f_is_the_shorter_mate"] = (mates(80, 100, 80), pp(20), [(80, 100, 80), (80, 80, 80)])
    cases["pair_f_is_the_shorter_mate_1"] = (mates(70, 70, 100), pp(20), [(70, 70, 70), (70, 100, 70)])
    cases["pair_f_at_top_minus_63"] = (mates(87, 150, 150), pp(20), [(87, 150, 87)] * 2)
    cases["pair_f_at_top_minus_64"] = (mates(86, 150, 150), pp(20), [(86, 150, 86)] * 2)
    cases["pair_f_in_the_third_group"] = (mates(21, 150, 151), pp(20), [(21, 150, 21), (21, 151, 21)])
    X = rand_letters(rnd, 30, b"ACG")
    cases["pair_two_lengths_the_greatest_wins"] = ([X + X + T(40), revcomp(X) + revcomp(X) + T(40)], pp(20),
                                                   [(60, 100, 60)] * 2)
    for f, ok, over in ((20, 2, 3), (30, 3, 4)):
        for k in (ok, over):
            frag = rand_letters(rnd, f, b"ACG")
            r1, r2 = mates(f, 100, 100, frag)
            r1 = bytearray(r1)
            for i in range(k):
                r1[1 + 4 * i] = ord("T")  # T against the fragment's complement of ACG: a mismatch
            want = [(f, 100, f)] * 2 if k == ok else [(100, 100, 0)] * 2
            cases[f"pair_threshold_f{f}_pm{k}"] = ([bytes(r1), r2], pp(20), want)
    frag = rand_letters(rnd, 40, b"ACG")
    r1, r2 = mates(40, 90, 90, frag)
    cases["pair_err_pct_0_exact"] = ([r1, r2], pp(20, 0), [(40, 90, 40)] * 2)
    cases["pair_N_on_mate_1"] = ([r1[:5] + b"N" + r1[6:], r2], pp(20, 0), [(90, 90, 0)] * 2)
    cases["pair_N_on_mate_2"] = ([r1, r2[:5] + b"N" + r2[6:]], pp(20, 0), [(90, 90, 0)] * 2)
    cases["pair_N_on_both_at_one_column"] = ([r1[:5] + b"N" + r1[6:], r2[:34] + b"N" + r2[35:]], pp(20, 0),
                                             [(90, 90, 0)] * 2)
    cases["pair_N_within_the_budget"] = ([r1[:5] + b"N" + r1[6:], r2[:5] + b"n" + r2[6:]], pp(20, 10),
                                         [(40, 90, 40)] * 2)
    cases["pair_lowercase"] = ([r1.lower(), r2], pp(20, 0), [(40, 90, 40)] * 2)
    big = rand_letters(rnd, 300, b"ACG")
    cases["pair_mates_of_1024_examined"] = (mates(300, 1024, 1024, big), pp(20), [(300, 1024, 300)] * 2)
    cases["pair_full_overlap_of_1024"] = (mates(1024, 1024, 1024), pp(20), [(1024, 1024, 1024)] * 2)
    cases["pair_mate_of_1025_skipped"] = (mates(300, 1025, 1024, big) + mates(300, 1024, 1025, big), pp(20),
                                          [(1025, 1025, 0), (1024, 1024, 0), (1024, 1024, 0), (1025, 1025, 0)])
    cases["pair_an_empty_mate"] = ([b"", rand_letters(rnd, 50), rand_letters(rnd, 50), b"", b"", b""], pp(1),
                                   [(0, 0, 0), (50, 50, 0), (50, 50, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)])
    cases["pair_poly_A_against_poly_T"] = ([b"A" * 150, b"T" * 150], pp(20), [(150, 150, 150)] * 2)
    # both rules: the minimum
    frag = rand_letters(rnd, 60, b"ACG")
    r1, r2 = frag + T(10) + AD + T(7), revcomp(frag) + AD + T(17)
    cases["both_rules_pair_is_shorter"] = ([r1, r2], P(AD, b"", 5, 10, 20), [(60, 70, 60), (60, 60, 60)])
    cases["pair_rule_alone_with_adapters_unset"] = ([r1, r2], pp(20), [(60, 110, 60)] * 2)
    inner = frag[:30] + AD[:12] + frag[42:]  # the fragment itself holds the 12-letter adapter at 30
    cases["both_rules_adapter_is_shorter"] = ([inner + T(40), revcomp(inner) + T(40)], P(AD[:12], b"", 12, 0, 20),
                                              [(30, 30, 60), (60, 100, 60)])
    return cases


def grid_stride_set(n_reads=4500, seed=5):
    """More reads than a launch has waves (4 x 1024): short reads, every third ending in the adapter's start."""
    rnd = random.Random(seed)
    reads = []
    for k in range(n_reads):
        n = k % 23
        read = rand_letters(rnd, n)
        reads.append(plant(read, n // 2, TRUSEQ) if k % 3 == 0 else read)
    return reads


def grid_stride_pairs(n_pairs=4200, seed=6):
    """More pairs than a launch has waves: short mates, every other pair read through."""
    rnd = random.Random(seed)
    reads = []
    for k in range(n_pairs):
        n1, n2 = 8 + k % 19, 8 + k % 17
        if k % 2:
            reads += list(read_through(rnd, rnd.randint(4, min(n1, n2)), n1, n2))
        else:
            reads += [rand_letters(rnd, n1), rand_letters(rnd, n2)]
    return reads


# ------------------------------------------------------------------ end to end on the golden testset
E2E_SINGLE = P(TRUSEQ, b"", 5, 10, 0)
E2E_PAIRS = P(TRUSEQ, TRUSEQ2, 5, 10, 20)


def e2e_reads(golden):
    """golden: name -> letters of the golden DNA reads (75 nt each). Returns (single, pairs): lists of (name, letters,
    planted) with planted the letters the read must keep. single: reads cut to a fragment and read through into the
    adapter (whole, as a tail to the read's end, followed by further letters, and with no fragment at all) among
    whole reads. pairs: records 2i and 2i + 1 are mates; two read-through pairs, a pair that overlaps fully
    (subject4 is subject3's reverse complement), a low-complexity pair, which accepts every length and keeps all, and
    a pair without overlap."""
    g = {k: v.encode() for k, v in golden.items()}
    assert all(len(g[k]) == 75 for k in ("subject0", "subject2", "subject3", "subject4"))
    assert g["subject4"] == revcomp(g["subject3"])
    single = [
        ("whole0", g["subject0"], 75),
        ("frag48", g["subject0"][:48] + TRUSEQ, 48),
        ("tail15", g["subject3"][:60] + TRUSEQ[:15], 60),
        ("whole2", g["subject2"], 75),
        ("frag30", g["subject4"][:30] + TRUSEQ + b"ACCGTTGACTGA", 30),
        ("dimer", TRUSEQ + b"ATCTCGTATGCCGTCTTCTGCTTG", 0),
        ("whole3", g["subject3"], 75),
    ]
    f0, f4 = g["subject0"][:50], g["subject4"][:40]
    pairs = [
        ("p0/1", f0 + TRUSEQ[:25], 50), ("p0/2", revcomp(f0) + TRUSEQ2[:25], 50),
        ("p1/1", g["subject3"], 75), ("p1/2", g["subject4"], 75),
        ("p2/1", g["subject2"], 75), ("p2/2", revcomp(g["subject2"]), 75),
        ("p3/1", f4 + TRUSEQ + b"AC", 40), ("p3/2", revcomp(f4) + TRUSEQ2 + b"GT", 40),
        ("p4/1", g["subject0"], 75), ("p4/2", g["subject4"], 75),
    ]
    return single, pairs


def check_e2e(single, pairs):
    """The model finds every planted cut exactly and cuts no unplanted read; returns its records and sums."""
    res = []
    for reads, params in ((single, E2E_SINGLE), (pairs, E2E_PAIRS)):
        out, sums = model_reads([r[1] for r in reads], params)
        assert out["kept"].tolist() == [r[2] for r in reads], (out["kept"].tolist(), [r[2] for r in reads])
        res.append((out, sums))
    out, _ = res[1]
    assert out["pair_len"].tolist() == [50, 50, 75, 75, 75, 75, 40, 40, 0, 0]
    return res


# ------------------------------------------------------------------ the refusals, by reason
REFUSALS = [
    ("param", dict(mo=0)), ("param", dict(mo=65)), ("param", dict(err=51)), ("param", dict(po=1025)),
    ("adapter", dict(a1=b"ACGU")), ("adapter", dict(a2=b"AC-T")), ("adapter", dict(a1=b"A" * 65)),
    ("adapter", dict(a1=b"ACGT", a2=b"C" * 65)),
    ("record", dict(offsets=[0, 99])), ("record", dict(lengths=[4, 95])), ("record", dict(offsets=[0, 1 << 40])),
    ("length", dict(big=True)),
    ("pairs", dict(po=20, offsets=[0, 10, 20], lengths=[4, 4, 4])),
    ("pairs", dict(po=20, a1=b"", offsets=[0], lengths=[4])),
]


def refusal_args(change):
    if change.get("big"):
        n = (1 << 24) + 1
        return (b"A" * n, [0], [n], b"ACGT", b"", 5, 10, 0)
    return (b"ACGT" * 25, change.get("offsets", [0, 50]), change.get("lengths", [4, 50]), change.get("a1", b"ACGTN"),
            change.get("a2", b""), change.get("mo", 5), change.get("err", 10), change.get("po", 0))


# ------------------------------------------------------------------ what the sets must hold
def check_sets():
    for m, mo, err in ADAPTER_SETS:
        reads, adapter = fixed_set(m, mo)
        assert len(adapter) == m and set(len(r) for r in reads) == set(FIXED_LENGTHS(mo))
        out, sums = model_reads(reads, P(adapter, b"", mo, err))
        if m >= mo:
            assert 0 < sums["adapter_found"] < len(reads), (m, mo, err)
        reads, adapter = random_set(m, mo, err)
        out, sums = model_reads(reads, P(adapter, b"", mo, err))
        lens = np.array([len(r) for r in reads])
        if m >= mo and (m, mo, err) != (64, 64, 50):
            assert (out["adapter_at"] < lens).sum() >= 40, (m, mo, err)
            # (a one-letter adapter is in every read of some length)
            assert (out["adapter_at"] == lens).sum() >= (20 if m >= 33 else 0), (m, mo, err)
        if m >= 33 and err:
            assert (out["adapter_mismatches"] > 0).sum() >= 10, (m, mo, err)
        letters, offs, lens = lay_out(reads, adapter)
        assert all(int(o) % 2 == 1 for o in offs)
    for po, err in PAIR_SETS:
        reads = random_pairs(po, err)
        out, sums = model_reads(reads, P(b"", b"", 5, err, po))
        assert 30 <= sums["pair_found"] <= len(reads) // 2 - 20 or err == 50, (po, err, sums)
        assert (out["pair_len"][0::2] == out["pair_len"][1::2]).all()
        if err:
            assert (out["pair_mismatches"] > 0).sum() >= 10
    cc = named_cases()
    for name, (reads, params, want) in cc.items():
        out, _ = model_reads(reads, params)
        if want is not None:
            got = [(int(o["kept"]), int(o["adapter_at"]), int(o["pair_len"])) for o in out]
            assert got == want, (name, got, want)
    assert len(grid_stride_set()) > 4 * 1024 and len(grid_stride_pairs()) // 2 > 4 * 1024
    out, sums = model_reads(grid_stride_pairs(), P(TRUSEQ, TRUSEQ2, 5, 10, 8))
    assert sums["pair_found"] > 500 and sums["adapter_found"] > 500
