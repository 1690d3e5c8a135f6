"""Cases and models of the tiled query sets (tests/test_gpu_query_tiles.py and
tests/tiles_poison_child.py; not a test module itself): the tile plan restated
in Python, a small model of the six-frame rule (the whole frame translated at
the read's own length, a stop blanks the frame until the next ATG, '*' past the
last whole codon, a tile is a slice), and the record cases."""
import numpy as np

AA = "ARNDCQEGHILKMFPSTWYV"
ORDER = "ARNDCQEGHILKMFPSTWYVBJZX*"  # residue codes 0..24; X is 23
CODONS = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"  # first base major over A C G T

_CODE = np.full(256, 23, dtype=np.uint8)
for _i, _c in enumerate(ORDER):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def code_record(letters: str, width: int) -> np.ndarray:
    """The coded record of a protein string: cut at the width, X-padded."""
    out = np.full(width, 23, dtype=np.uint8)
    b = np.frombuffer(letters[:width].encode(), dtype=np.uint8)
    out[:len(b)] = _CODE[b]
    return out


def residues(codes: np.ndarray) -> np.ndarray:
    """The query length of every row: last non-X code + 1, at least 1."""
    nonx = codes != 23
    last = codes.shape[1] - np.argmax(nonx[:, ::-1], axis=1)
    return np.where(nonx.any(axis=1), last, 1).astype(np.uint32)


def starts(m: int, W: int, step: int) -> list:
    if m <= W:
        return [0]
    tiles = 1 + -(-(m - W) // step)
    return [t * step for t in range(tiles - 1)] + [m - W]


def six_frames(read: str) -> list:
    """The six frames of a read at its own length n: n // 3 letters each."""
    n = len(read)
    base = {"A": 0, "C": 1, "G": 2, "T": 3}
    fwd = [base.get(c.upper(), 5 if c == "-" else 4) for c in read]
    rev = [b if b > 3 else 3 - b for b in reversed(fwd)]
    frames = []
    for strand in (fwd, rev):
        for off in range(3):
            p, stop = [], False
            for k in range(off + 2, n, 3):
                b = strand[k - 2:k + 1]
                if max(b) > 3:
                    letter = "X"
                else:
                    codon = b[0] << 4 | b[1] << 2 | b[2]
                    if codon == 14:
                        stop = False
                    elif codon in (48, 50, 56):
                        stop = True
                    letter = CODONS[codon]
                p.append("*" if stop else letter)
            frames.append("".join(p) + "*" * (n // 3 - len(p)))
    return frames


def protein_tiles(recs, W, step, max_len=0):
    """[(name, letters of the tile, source record, offset, source letters)] in output order."""
    out = []
    for r, (name, seq) in enumerate(recs):
        kept = seq[:max_len] if max_len else seq
        for s in starts(len(kept), W, step):
            out.append((name, kept[s:s + W], r, s, len(kept)))
    return out


def dna_tiles(recs, W, step, max_len=0):
    """[(name, letters of the tile, source record, offset, frame letters, frame)]: tile-major, frame-minor."""
    out = []
    for r, (name, seq) in enumerate(recs):
        kept = seq[:max_len] if max_len else seq
        frames = six_frames(kept)
        m = len(kept) // 3
        for s in starts(m, W, step):
            for f in range(6):
                out.append((name, frames[f][s:s + W], r, s, m, f))
    return out


def protein_lengths(W, step, max_len):
    lens = []
    for n in (0, 1, W - 1, W, W + 1, W + step - 1, W + step, W + step + 1, 2 * W - 1, 2 * W, 3 * W + 5, max_len,
              max_len + 1):
        if n >= 0 and n not in lens:
            lens.append(n)
    return lens


def protein_records(W, step, max_len, r):
    """Records of every length at which the plan or the kernel takes another
    path, and the letter oddities of test_gpu_set_queries.protein_fasta."""
    rand = lambda n: "".join(r.choice(AA) for _ in range(n))  # noqa: E731
    recs = [(f"len{n}", rand(n)) for n in protein_lengths(W, step, max_len)]
    recs += [("only_x", "XXX"), ("ends_in_x", "MK" + "xUO"), ("lower_unknown", "acdefBZJ*u1-wy"),
             ("tail_x_long", rand(max(W - 3, 1)) + "XXXXXX"), ("x_run_over_a_tile", rand(5) + "X" * (W + step) + rand(3)),
             ("long_lower", rand(2 * W + 7).lower()), ("last", rand(W // 2 + 1))]
    return recs


PROTEIN_CASES = [(W, step) for W in (63, 64, 65, 127) for step in sorted({1, W // 2, W - 1, W})]


def dna_records(W, step, r):
    """Reads (nt) for frame width W letters and tile step `step`."""
    rand = lambda n: "".join(r.choice("ACGT") for _ in range(n))  # noqa: E731
    quiet = lambda n: "GCT" * n  # noqa: E731  (A in frame 0, no stop or ATG in any frame)
    # (a read of over 170 tiles is refused: 15 W + 1 nt only where the step allows it)
    recs = [(f"n{n}", rand(n)) for n in (3 * W - 1, 3 * W, 3 * W + 1, 3 * W + 2, 3 * W + 3, 3 * (W + step) + 2,
                                         15 * W + 1) if len(starts(n // 3, W, step)) <= 170]
    # frame 0: a stop in the letter just before the second tile's start, without and with an ATG inside that tile
    recs.append(("stop_before_tile", quiet(step - 1) + "TAA" + quiet(W + 5)))
    recs.append(("stop_before_tile_atg", quiet(step - 1) + "TAA" + quiet(3) + "ATG" + quiet(W + 1)))
    # stop on letter 63 and ATG on letter 64 of frame 0 (the 64-letter group's edge), and the other way round
    recs.append(("stop63_atg64", quiet(63) + "TAA" + "ATG" + quiet(W + 70)))
    recs.append(("atg63_stop64", "TAG" + quiet(62) + "ATG" + "TGA" + quiet(W + 70)))
    # TTA: a stop (TAA) on the reverse strand only
    recs.append(("reverse_stop", "CCG" * 20 + "TTA" + "CCG" * (W + 40)))
    with_n = list(rand(3 * (W + step) + 10))
    for k in range(0, len(with_n), 7):
        with_n[k] = "N"
    recs.append(("with_n", "".join(with_n)))
    recs.append(("lower_gap", "atg-ry" + rand(3 * W + 40).lower()))
    recs.append(("stops", "TAATAGTGA" * (W // 2)))
    recs.append(("empty", ""))
    recs.append(("two_bases", "AC"))
    recs.append(("last", rand(3 * W + 17)))
    return recs


DNA_CASES = [(127, 64), (127, 1), (65, 32), (64, 64), (63, 62), (40, 7)]
