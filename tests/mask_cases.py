"""Cases and the model of the low-complexity mask (tests/test_query_mask_host.py,
tests/test_gpu_query_mask.py and tests/mask_poison_child.py; not a test module
itself).

The model is the rule restated letter by letter over a list of codes:
T[c] = round(1024 c log2 c); window i covers letters [i, i + w) and is evaluated
when all its codes are below 23; S = sum of T[count], d = 100 (T[w] - S); low
when d <= k2 1024 w, a trigger when d <= k1 1024 w; a maximal run of low windows
i..j with a trigger masks letters [i, j + w). A masked letter becomes 23 in
every tile record that covers it.

A case set is one (W, step, stride) layout of tile records with sources of every
letter count in M_VALUES, some clean, some with planted stretches; every set is
checked on the model's own output: at least a third of its sources masked, at
least a third untouched."""
import functools
import math
import random
from collections import Counter

import numpy as np

X, STAR = 23, 24
M_VALUES = lambda w: [w - 1, w, w + 1, 63, 64, 65, 63 + w, 64 + w - 1, 64 + w, 200]  # noqa: E731
WINDOWS = (6, 12, 32)
LEVELS = ((220, 250), (0, 0), (250, 250), (0, 500))
# (W, step, stride): tiled protein sources (tiles next to each other) and DNA frames (tiles six records apart), and
# an untiled set (every record its own source of W letters, the step the width)
LAYOUTS = [(W, step, stride) for W, step in ((20, 7), (64, 64), (127, 64), (127, 1)) for stride in (1, 6)]
UNTILED = (75, 75, 0)
SOURCE_DTYPE = [("first_record", "<u4"), ("stride", "<u4"), ("tiles", "<u4"), ("letters", "<u4")]


# ------------------------------------------------------------------ the model
def table(w):
    return [0] + [int(math.floor(1024 * c * math.log2(c) + 0.5)) for c in range(1, w + 1)]


def flags(codes, w, k1, k2):
    """(low, trigger) per window of a list of codes."""
    T = table(w)
    low, trig = [], []
    for i in range(len(codes) - w + 1):
        win = codes[i:i + w]
        if max(win) >= X:
            low.append(False)
            trig.append(False)
            continue
        d = 100 * (T[w] - sum(T[n] for n in Counter(win).values()))
        low.append(d <= k2 * 1024 * w)
        trig.append(d <= k1 * 1024 * w)
    return low, trig


def mask_letters(codes, w, k1, k2):
    """Which letters of a source are masked."""
    codes = [int(c) for c in codes]
    out = [False] * len(codes)
    low, trig = flags(codes, w, k1, k2)
    i = 0
    while i < len(low):
        if not low[i]:
            i += 1
            continue
        j = i
        while j + 1 < len(low) and low[j + 1]:
            j += 1
        if any(trig[i:j + 1]):
            for p in range(i, j + w):
                out[p] = True
        i = j + 1
    return out


def starts(m, W, step):
    if m <= W:
        return [0]
    tiles = 1 + -(-(m - W) // step)
    return [t * step for t in range(tiles - 1)] + [m - W]


def source_rows(src, W, step):
    """[(record, start)] of a source's tiles."""
    first, stride, tiles, m = (int(src[k]) for k in ("first_record", "stride", "tiles", "letters"))
    st = starts(m, W, step)
    assert len(st) == tiles
    return [(first + (stride * t if tiles > 1 else 0), s) for t, s in enumerate(st)]


def read_source(records, src, W, step):
    """A source's letters through the tile table: letter p from tile min(p // step, tiles - 1)."""
    rows = source_rows(src, W, step)
    m = int(src["letters"])
    out = []
    for p in range(m):
        rec, s = rows[min(p // step, len(rows) - 1)]
        out.append(int(records[rec, p - s]))
    return out


def model(records, srcs, W, step, w, k1, k2):
    """(masked records, masked letters per record, masked letters per source) by the rule."""
    records = np.asarray(records, dtype=np.uint8).reshape(-1, W)
    out = records.copy()
    counts = np.zeros(len(records), dtype=np.uint32)
    per_source = []
    for src in srcs:
        m = int(src["letters"])
        if m < w:
            per_source.append(0)
            continue
        mask = mask_letters(read_source(records, src, W, step), w, k1, k2)
        per_source.append(sum(mask))
        for rec, s in source_rows(src, W, step):
            for k in range(min(W, m - s)):
                if mask[s + k]:
                    out[rec, k] = X
                    counts[rec] += 1
    return out, counts, per_source


# ------------------------------------------------------------------ the generator
def clean(r, m):
    """m letters with no two equal ones within 23 letters: a shuffled cycle of the codes 0..22."""
    cyc = list(range(23))
    r.shuffle(cyc)
    at = r.randrange(23)
    return [cyc[(at + p) % 23] for p in range(m)]


def stretch(r, kind, n):
    if kind == "homo":
        return [r.randrange(20)] * n
    if kind in ("per2", "per3"):
        unit = r.sample(range(20), 2 if kind == "per2" else 3)
        return [unit[p % len(unit)] for p in range(n)]
    pool = r.sample(range(23), 4 if kind == "four" else 6)  # entropy at most 2.0, and at most 2.585
    return [r.choice(pool) for _ in range(n)]


def planted(r, m, w, sprinkle):
    """Clean or random letters with planted stretches, X and '*' sprinkled into them or not, and last a
    homopolymer of at least w letters (masked at every pair of levels) when it fits."""
    s = clean(r, m) if r.random() < 0.5 else [r.randrange(20) for _ in range(m)]
    for _ in range(r.randrange(1, 4)):
        n = min(m, r.randrange(w, 3 * w + 8))
        at = r.randrange(m - n + 1)
        s[at:at + n] = stretch(r, r.choice(["homo", "per2", "per3", "four", "six", "six"]), n)
    if sprinkle:
        for _ in range(1 + m // 40):
            s[r.randrange(m)] = r.choice([X, STAR])
    if m >= w:
        n = min(m, r.randrange(w, w + 6))
        at = r.randrange(m - n + 1)
        s[at:at + n] = stretch(r, "homo", n)
    return s


def sources_of(r, m, w):
    """The letters of one letter count's sources: clean, planted (plain, sprinkled), clean with X and '*', random."""
    sprinkled = clean(r, m)
    for _ in range(1 + m // 50):
        sprinkled[r.randrange(m)] = r.choice([X, STAR])
    return [clean(r, m), planted(r, m, w, False), planted(r, m, w, True), sprinkled,
            [r.randrange(20) for _ in range(m)], planted(r, m, w, r.random() < 0.5)]


def lay_out(letter_lists, W, step, stride):
    """Tile records of the sources' letters: (records[n, W], sources). stride 1: a source's tiles consecutive;
    stride 6: six sources of one letter count share a block, tile t of source f at 6 t + f; stride 0: untiled,
    every record its own source of W letters (the letters cut at W, X behind them)."""
    rows, srcs = [], []
    if stride == 0:
        for s in letter_lists:
            rows.append((list(s[:W]) + [X] * W)[:W])
            srcs.append((len(rows) - 1, 1, 1, W))
    elif stride == 1:
        for s in letter_lists:
            st = starts(len(s), W, step)
            srcs.append((len(rows), 1, len(st), len(s)))
            rows += [(list(s[a:a + W]) + [X] * W)[:W] for a in st]
    else:
        assert len(letter_lists) % 6 == 0
        for b in range(0, len(letter_lists), 6):
            block = letter_lists[b:b + 6]
            m = len(block[0])
            assert all(len(s) == m for s in block)
            st = starts(m, W, step)
            base = len(rows)
            for a in st:
                rows += [(list(s[a:a + W]) + [X] * W)[:W] for s in block]
            srcs += [(base + f, 6, len(st), m) for f in range(6)]
    return np.array(rows, dtype=np.uint8).reshape(-1, W), np.array(srcs, dtype=SOURCE_DTYPE)


@functools.lru_cache(maxsize=None)
def case_set(w, levels, layout):
    """(records, sources, step, model records, model counts, model letters per source) of one case set."""
    W, step, stride = layout
    k1, k2 = levels
    r = random.Random(hash((w, k1, k2, W, step, stride)) & 0xFFFFFFFF)
    letters = []
    for m in M_VALUES(w):
        letters += sources_of(r, m, w)
    records, srcs = lay_out(letters, W, step, stride)
    want, counts, per_source = model(records, srcs, W, step, w, k1, k2)
    some = sum(1 for n in per_source if n)
    # a set in which nothing, or everything, is masked proves nothing
    assert 3 * some >= len(srcs) and 3 * (len(srcs) - some) >= len(srcs), (w, levels, layout, some, len(srcs))
    return records, srcs, step, want, counts, per_source


def all_case_sets():
    return [(w, lv, lay) for w in WINDOWS for lv in LEVELS for lay in LAYOUTS + [UNTILED]]


# ------------------------------------------------------------------ the carry cases, by name
def carry_cases():
    """name -> (letter lists, W, step, stride, w, (k1, k2), check): check(low, trigger, mask) of the first
    source asserts on the model's own flags that the case is what its name says."""
    r = random.Random(20240607)
    w = 12
    out = {}

    def runs_of(low):
        runs, i = [], 0
        while i < len(low):
            if low[i]:
                j = i
                while j + 1 < len(low) and low[j + 1]:
                    j += 1
                runs.append((i, j))
                i = j + 1
            else:
                i += 1
        return runs

    # a segment across letters 63 / 64
    s = clean(r, 130)
    s[58:72] = [4] * 14

    def across(low, trig, mask):
        assert mask[63] and mask[64] and not mask[40] and not mask[100]
    out["across_63_64"] = ([s], 127, 64, 1, w, (220, 250), across)

    # a low run over three 64-window groups, its triggers in the first group only / in the last only: a period-5
    # repeat (counts 3 3 2 2 2 in every window, 2.29 bits: low, no trigger) beside a period-4 one (2.0 bits)
    p5 = [[0, 1, 2, 3, 5][p % 5] for p in range(230)]
    p4 = [[0, 1, 2, 3][p % 4] for p in range(16)]
    for name, s in (("trigger_in_first_group", p4 + p5 + clean(r, 30)), ("trigger_in_last_group", clean(r, 70) + p5 + p4)):
        def spans(low, trig, mask, name=name):
            run = max(runs_of(low), key=lambda x: x[1] - x[0])
            groups = {i // 64 for i in range(run[0], run[1] + 1) if trig[i]}
            assert run[1] // 64 - run[0] // 64 >= 2 and len(groups) == 1
            assert groups == ({run[0] // 64} if name == "trigger_in_first_group" else {run[1] // 64})
            assert all(mask[run[0]:run[1] + w])
        out[name] = ([s], 127, 64, 1, w, (220, 250), spans)

    # a segment ending at m - 1
    s = clean(r, 90)
    s[-15:] = [7] * 15

    def at_end(low, trig, mask):
        assert mask[-1] and low[-1] and not mask[30]
    out["ends_at_m_minus_1"] = ([s], 64, 20, 1, w, (220, 250), at_end)

    # two segments exactly w - 1 windows apart, so that their masks touch: at levels (0, 0) only a window of one
    # letter is low, so a run of A's and a run of C's next to it are two segments
    s = clean(r, 20) + [0] * 14 + [4] * 13 + clean(r, 25)

    def touch(low, trig, mask):
        a, b = runs_of(low)
        assert b[0] - a[1] == w and all(mask[a[0]:b[1] + w]) and not mask[a[0] - 1] and not mask[b[1] + w]
    out["masks_touch"] = ([s], 127, 64, 1, w, (0, 0), touch)

    # the flush-right last tile (start m - W = 17, its neighbour's 14) with a segment inside their overlap
    s = clean(r, 37)
    s[18:33] = [9] * 15

    def flush(low, trig, mask):
        assert starts(37, 20, 7) == [0, 7, 14, 17] and all(mask[18:33]) and not mask[10]
    out["flush_right_overlap"] = ([s], 20, 7, 1, w, (220, 250), flush)
    return out


DNA_READ = "GATTACAGGCTTACCGATGC" * 3 + "CAG" * 14 + "TAA" + "CAG" * 5 + "ATG" + "CAG" * 14 + "TTGACCGTAGGCTAACGT" * 4


def dna_carry_case():
    """All six frames of a DNA read with a stop run in the middle of a low stretch: the letters of its frames."""
    import tile_cases as tc

    frames = tc.six_frames(DNA_READ)
    code = {c: i for i, c in enumerate(tc.ORDER)}
    return [[code[c] for c in f] for f in frames]


# ------------------------------------------------------------------ refusals
# (reason, what differs from: four records of 20 letters, src [(0, 1, 3, 30)], step 5, window 12, levels 220 / 250)
REFUSALS = [
    ("window", dict(window=5)), ("window", dict(window=33)), ("window", dict(window=0)),
    ("levels", dict(trigger=251)), ("levels", dict(extend=501, trigger=0)), ("levels", dict(trigger=300, extend=200)),
    ("source", dict(step=0)), ("source", dict(step=21)),
    ("source", dict(src=[(0, 1, 0, 30)])), ("source", dict(src=[(0, 1, 1, 0)])), ("source", dict(src=[(0, 1, 2, 30)])),
    ("source", dict(src=[(0, 0, 3, 30)])), ("source", dict(src=[(2, 1, 3, 30)])), ("source", dict(src=[(4, 1, 1, 20)])),
    ("overlap", dict(src=[(0, 1, 3, 30), (2, 1, 1, 20)])), ("overlap", dict(src=[(1, 1, 1, 20), (1, 1, 1, 12)])),
]


def refusal_args(change):
    args = dict(src=[(0, 1, 3, 30)], step=5, window=12, trigger=220, extend=250)
    args.update(change)
    return np.full((4, 20), 5, dtype=np.uint8), np.array(args["src"], dtype=SOURCE_DTYPE), args


# ------------------------------------------------------------------ session sets
ORDER = "ARNDCQEGHILKMFPSTWYVBJZX*"


def letters_of(codes):
    return "".join(ORDER[c] for c in codes)


def session_sets():
    """name -> (seqs, names, set_queries keywords, W, step or None): an untiled protein set, a tiled protein set
    and a tiled DNA set, each with planted and clean records."""
    r = random.Random(77)
    w = 12
    prot = [letters_of(s) for m in (11, 12, 40, 75, 90) for s in sources_of(r, m, w)]
    long = [letters_of(s) for m in (11, 64, 65, 150, 301) for s in sources_of(r, m, w)]
    nt = lambda n: "".join(r.choice("ACGT") for _ in range(n))  # noqa: E731
    dna = [DNA_READ, nt(30), nt(400), nt(121) + "GCA" * 30 + nt(77), "A" * 90 + nt(200), nt(250) + "CTG" * 25, nt(500), "AC", ""]
    dna += [nt(n) for n in (120, 150, 200, 260, 390, 391)]
    name = lambda k, xs: [f"{k}{i}" for i in range(len(xs))]  # noqa: E731
    return {
        "protein_untiled": (prot, name("p", prot), dict(width=75), 75, None),
        "protein_tiled": (long, name("t", long), dict(width=64, tile_step=20), 64, 20),
        "dna_tiled": (dna, name("d", dna), dict(width=120, dna=True, tile_step=13), 40, 13),
    }


def session_sources(tiles, nrec, W, dna):
    """The sources the session masks: every record of an untiled set (tiles empty) with W letters; of a tiled set
    every (record, frame) of the tile table that has a letter."""
    if len(tiles) == 0:
        return np.array([(i, 1, 1, W) for i in range(nrec)], dtype=SOURCE_DTYPE)
    first = {}
    for i, t in enumerate(tiles):
        key = (int(t["record"]), int(t["frame"]))
        if key not in first:
            first[key] = [i, 0, int(t["letters"])]
        first[key][1] += 1
    return np.array([(i, 6 if dna else 1, n, m) for i, n, m in first.values() if m > 0], dtype=SOURCE_DTYPE)
