"""Tiled query sets (GhostmSessionSetQueries*Tiled, `ghostm search -T`): reads
longer than one record enter the search as overlapping tile records under their
name, made on the GPU by the tiled kernels of qformat.hip.

Record level: the protein tiles against the untiled setter run on the explicit
substrings, the DNA tiles against a Python model of the six-frame rule (first
checked itself against the untiled setter), lengths against last-non-X + 1,
the tile table against the plan. Search level: a tiled set against the same
tiles given explicitly under repeated names (hits and text byte-equal), the
detail lines with the tile's offset added, and every refusal leaving the old
set in place."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cases
import tile_cases as tc
from ghostm_amd import GhostmError, native, tile_plan
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db_session(dataset):
    d = dataset("protein_testset")
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        yield s


def all_records(s, width):
    """Every query record of the session, over its chunks: codes[n, width]."""
    out, c = [], 0
    total = len(s.query_lengths())
    while sum(len(x) for x in out) < total:
        out.append(s.query_records(c).reshape(-1, width))
        c += 1
    return np.concatenate(out) if out else np.zeros((0, width), dtype=np.uint8)


def table_of(tiles):
    return [(int(t["record"]), int(t["offset"]), int(t["letters"]), int(t["frame"])) for t in tiles]


# ------------------------------------------------------------------ record level
@pytest.mark.parametrize("W,step", tc.PROTEIN_CASES)
def test_protein_tiles(db_session, W, step):
    s = db_session
    max_len = 2 * W + step + 3
    recs = tc.protein_records(W, step, max_len, random.Random(W * 1000 + step))
    want = tc.protein_tiles(recs, W, step, max_len)
    # the untiled setter on the explicit substrings
    s.set_queries([t[1] for t in want], [t[0] for t in want], width=W)
    assert len(s.query_tiles()) == 0
    explicit = all_records(s, W)
    explicit_len = s.query_lengths()
    s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=W, tile_step=step, max_len=max_len)
    got = all_records(s, W)
    assert got.shape == explicit.shape == (len(want), W)
    assert got.tobytes() == explicit.tobytes()
    assert got.tobytes() == np.stack([tc.code_record(t[1], W) for t in want]).tobytes()
    assert s.query_lengths().tolist() == tc.residues(got).tolist() == explicit_len.tolist()
    tiles = s.query_tiles()
    assert table_of(tiles) == [(t[2], t[3], t[4], 0) for t in want]
    plan, cut = tile_plan([len(x[1]) for x in recs], width=W, step=step, max_len=max_len)
    assert plan.tobytes() == tiles.tobytes()
    assert cut == sum(len(x[1]) > max_len for x in recs) > 0


def test_model_equals_untiled_setter(db_session):
    """The six-frame model itself: reads of one length n with n / 3 <= W against
    the untiled setter's records."""
    s = db_session
    for n in (190, 191, 192, 381):
        r = random.Random(n)
        reads = [(name, (seq + "".join(r.choice("ACGT") for _ in range(n)))[:n])
                 for name, seq in tc.dna_records(60, 30, r) if name != "empty"]
        s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=381, dna=True)
        got = all_records(s, 127)
        want = np.stack([tc.code_record(f, 127) for _, seq in reads for f in tc.six_frames(seq)])
        assert got.tobytes() == want.tobytes(), n


@pytest.mark.parametrize("W,step", tc.DNA_CASES)
def test_dna_tiles(db_session, W, step):
    s = db_session
    recs = tc.dna_records(W, step, random.Random(W * 1000 + step))
    for max_len in (0, 3 * (W + step) + 1):
        want = tc.dna_tiles(recs, W, step, max_len)
        s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=3 * W, dna=True, tile_step=step,
                      max_len=max_len)
        got = all_records(s, W)
        assert got.shape == (len(want), W)
        model = np.stack([tc.code_record(t[1], W) for t in want])
        bad = np.nonzero((got != model).any(axis=1))[0]
        assert bad.size == 0, [(want[k][0], want[k][3], want[k][5]) for k in bad[:5]]
        assert s.query_lengths().tolist() == tc.residues(got).tolist()
        tiles = s.query_tiles()
        assert table_of(tiles) == [(t[2], t[3], t[4], t[5]) for t in want]
        plan, cut = tile_plan([len(x[1]) for x in recs], width=3 * W, dna=True, step=step, max_len=max_len)
        assert plan.tobytes() == tiles.tobytes()
        assert cut == (6 * sum(len(x[1]) > max_len for x in recs) if max_len else 0)


def test_dna_stop_carried_into_tiles(db_session):
    """The crafted reads as codes: a stop just before a tile's start blanks the
    tile's head until its ATG; stop and ATG on letters 63 and 64."""
    s = db_session
    W, step = 127, 50
    recs = [x for x in tc.dna_records(W, step, random.Random(1)) if x[0] in
            ("stop_before_tile", "stop_before_tile_atg", "stop63_atg64", "atg63_stop64")]
    s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=3 * W, dna=True, tile_step=step)
    got = all_records(s, W)
    tiles = s.query_tiles()
    row = lambda r, t: got[[k for k, x in enumerate(tiles) if x["record"] == r and x["frame"] == 0][t]]  # noqa: E731
    star, ala, met = 24, 0, 12
    assert row(0, 0)[:step].tolist() == [ala] * (step - 1) + [star]
    assert (row(0, 1) == star).all()                      # no ATG: blank to the tile's end
    assert row(1, 1)[:6].tolist() == [star] * 3 + [met, ala, ala]
    assert row(2, 0)[61:67].tolist() == [ala, ala, star, met, ala, ala]
    t1 = row(2, 1)                                        # starts at letter 50: letters 63, 64 are bytes 13, 14
    assert tiles[[k for k, x in enumerate(tiles) if x["record"] == 2][6]]["offset"] == 50
    assert t1[11:17].tolist() == [ala, ala, star, met, ala, ala]
    assert row(3, 0)[:3].tolist() == [star] * 3 and row(3, 0)[62:66].tolist() == [star, met, star, star]


def test_fasta_setter_equals_record_setter(db_session, tmp_path):
    s = db_session
    recs = [x for x in tc.protein_records(64, 32, 150, random.Random(5)) if x[1]]
    with open(tmp_path / "p.fa", "w") as f:
        for name, seq in recs:
            f.write(f">{name}\n{seq}\n")
    s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=64, tile_step=32, max_len=150)
    want = (all_records(s, 64).tobytes(), s.query_lengths().tolist(), s.query_tiles().tobytes())
    cut = s.set_queries_fasta(str(tmp_path / "p.fa"), width=64, tile_step=32, max_len=150)
    assert cut == sum(len(x[1]) > 150 for x in recs)
    assert (all_records(s, 64).tobytes(), s.query_lengths().tolist(), s.query_tiles().tobytes()) == want
    assert s.stats()["seconds_query_format"] > 0 and s.stats()["seconds_query_read"] > 0


# ------------------------------------------------------------------ degenerate equality
@pytest.mark.parametrize("style", ["0", "1", "2"])
def test_no_long_record_equals_untiled(dataset, style):
    """No record over the width: the tiled setter's records, lengths and text
    are the untiled setter's bytes."""
    d = dataset("syn_small")
    r = random.Random(11)
    subjects = [x[1] for x in fasta_records(os.path.join(d, "db.fa")) if len(x[1]) >= 100]
    piece = lambda i, n: mutate(subjects[i % len(subjects)][20:20 + n], r)  # noqa: E731
    protein = [(f"p{i}", piece(i, r.randint(1, 60))) for i in range(40)]
    dna = [(f"d{i}", back_translate(piece(i, 60), r)) for i in range(40)]
    hits = 0
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0", "-y", style]) as s:
        for recs, kw in ((protein, dict(width=60)), (dna, dict(width=180, dna=True))):
            seqs, names = [x[1] for x in recs], [x[0] for x in recs]
            s.set_queries(seqs, names, **kw)
            s.run()
            want = (s.query_records(0).tobytes(), s.query_lengths().tolist(), s.output(), s.hits().tobytes())
            s.set_queries(seqs, names, tile_step=7, **kw)
            s.run()
            assert (s.query_records(0).tobytes(), s.query_lengths().tolist(), s.output(), s.hits().tobytes()) == want
            assert len(s.query_tiles()) == len(want[1])
            hits += len(s.hits())
        assert hits > 0


# ------------------------------------------------------------------ search level
def mutate(seq, r, rate=0.08):
    return "".join(r.choice(tc.AA) if r.random() < rate else c for c in seq)


def fasta_records(path):
    out = []
    for block in open(path).read().split(">")[1:]:
        name, _, seq = block.partition("\n")
        out.append((name.strip(), seq.replace("\n", "")))
    return out


@pytest.fixture(scope="module")
def long_reads(dataset):
    """Protein reads of up to about 400 aa: stretches of syn_small subjects,
    mutated, between random flanks, so the homology lies anywhere in the read."""
    d = dataset("syn_small")
    subjects = [x for x in fasta_records(os.path.join(d, "db.fa")) if len(x[1]) >= 150]
    r = random.Random(2024)
    rand = lambda n: "".join(r.choice(tc.AA) for _ in range(n))  # noqa: E731
    reads = []
    for i in range(60):
        sub = subjects[(i * 7) % len(subjects)][1]
        a = r.randrange(0, len(sub) - 100)
        core = mutate(sub[a:a + r.randint(60, 200)], r)
        reads.append((f"read{i}", (rand(r.randint(0, 150)) + core + rand(r.randint(0, 120)))[:400]))
    reads.append(("short", mutate(subjects[3][1][:90], r)))
    reads.append(("random", rand(391)))
    return reads


def run_pair(d, opts, tiled_call, explicit_call, env=None):
    """(tiled session results, explicit-tile session results): output, hits,
    hits_rows query records, tile table."""
    out = []
    for call in (tiled_call, explicit_call):
        with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"] + opts) as s:
            call(s)
            s.run()
            res = dict(output=s.output(), hits=s.hits(), tiles=s.query_tiles(), chunks=s.stats()["query_format_launches"])
            if opts[:1] == ["-y"] and opts[1] in ("6", "8"):
                res["rows"] = s.hits_rows()[0]
            out.append(res)
    return out


SEARCH_CASES = [("default", [], 0, None), ("y2_b20", ["-y", "2", "-b", "20"], 0, None),
                ("one_lane_k4", [], 0, "4")]


@pytest.mark.parametrize("name,opts,chunk_mb,k4cap", SEARCH_CASES, ids=[c[0] for c in SEARCH_CASES])
def test_protein_search_equals_explicit_tiles(dataset, long_reads, monkeypatch, name, opts, chunk_mb, k4cap):
    d = dataset("syn_small")
    W, step = 127, 64
    want = tc.protein_tiles(long_reads, W, step)
    if k4cap:
        monkeypatch.setenv("GHOSTM_K4_CAP", k4cap)  # groups of more keys take K4's one-lane path
    tiled, explicit = run_pair(
        d, opts,
        lambda s: s.set_queries([x[1] for x in long_reads], [x[0] for x in long_reads], width=W, tile_step=step),
        lambda s: s.set_queries([t[1] for t in want], [t[0] for t in want], width=W))
    assert len(tiled["hits"]) > 30
    assert tiled["output"] == explicit["output"]
    assert tiled["hits"].tobytes() == explicit["hits"].tobytes()
    # a homology past the first record is found: some hit's group has a later tile
    assert len(tiled["tiles"]) == len(want) and len(explicit["tiles"]) == 0


def test_two_query_chunks(dataset, long_reads):
    """-c 1: the tiled set over two chunks (cut over the kept letters, a read's
    tiles never straddling), the explicit tiles in one."""
    d = dataset("syn_small")
    W, step = 127, 64
    r = random.Random(77)
    filler = [(f"fill{i}", "".join(r.choice(tc.AA) for _ in range(400))) for i in range(2700)]
    reads = long_reads[:20] + filler + long_reads[20:]
    want = tc.protein_tiles(reads, W, step)
    tiled, explicit = run_pair(
        d, [],
        lambda s: s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=W, tile_step=step, chunk_mb=1),
        lambda s: s.set_queries([t[1] for t in want], [t[0] for t in want], width=W))
    assert tiled["chunks"] == 2 and explicit["chunks"] == 1
    assert len(tiled["hits"]) > 30
    assert tiled["output"] == explicit["output"]
    assert tiled["hits"].tobytes() == explicit["hits"].tobytes()
    assert table_of(tiled["tiles"]) == [(t[2], t[3], t[4], 0) for t in want]


def back_translate(protein, r):
    by_aa = {}
    for k, aa in enumerate(tc.CODONS):
        by_aa.setdefault(aa, []).append("".join("ACGT"[(k >> s) & 3] for s in (4, 2, 0)))
    return "".join(r.choice(by_aa[a]) for a in protein)


def test_dna_search_equals_translated_tiles(dataset, long_reads):
    """DNA reads of up to 1200 nt, tiled, against the model's translated tiles
    given to the untiled protein setter under the same names."""
    d = dataset("syn_small")
    W, step = 127, 64
    r = random.Random(9)
    reads = [(name, "ACGT"[:r.randrange(3)] + back_translate(seq, r)) for name, seq in long_reads[::3]]
    reads += [(name + "_rc", back_translate(seq, r)[::-1].translate(str.maketrans("ACGT", "TGCA")))
              for name, seq in long_reads[1:12:3]]
    want = tc.dna_tiles(reads, W, step)
    tiled, explicit = run_pair(
        d, ["-y", "2"],
        lambda s: s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=3 * W, dna=True, tile_step=step),
        lambda s: s.set_queries([t[1] for t in want], [t[0] for t in want], width=W))
    assert len(tiled["hits"]) > 10
    assert tiled["output"] == explicit["output"]
    assert tiled["hits"].tobytes() == explicit["hits"].tobytes()


@pytest.mark.parametrize("style", ["6", "8"])
def test_detail_lines_in_read_coordinates(dataset, long_reads, style):
    """-y 6 and -y 8: every line is the explicit-tile session's with the tile's
    offset added to qstart and qend (columns 7 and 8)."""
    d = dataset("syn_small")
    W, step = 127, 64
    want = tc.protein_tiles(long_reads, W, step)
    tiled, explicit = run_pair(
        d, ["-y", style],
        lambda s: s.set_queries([x[1] for x in long_reads], [x[0] for x in long_reads], width=W, tile_step=step),
        lambda s: s.set_queries([t[1] for t in want], [t[0] for t in want], width=W))
    got, base = tiled["output"].split(b"\n"), explicit["output"].split(b"\n")
    assert len(got) == len(base) == len(tiled["hits"]) + 1 > 30
    assert tiled["rows"]["query_record"].tolist() == explicit["rows"]["query_record"].tolist()
    offsets = tiled["tiles"]["offset"][tiled["rows"]["query_record"]]
    assert (offsets > 0).any() and (offsets == 0).any()
    for line, plain, off in zip(got, base, offsets.tolist()):
        cols = plain.split(b"\t")
        cols[6], cols[7] = b"%d" % (int(cols[6]) + off), b"%d" % (int(cols[7]) + off)
        assert line == b"\t".join(cols)


def test_pairwise_view_in_read_coordinates(dataset, long_reads):
    """-y 9: the '#' line's qstart and qend and the Query row's two coordinates
    carry the offset; everything else is the explicit-tile session's."""
    d = dataset("syn_small")
    W, step = 127, 64
    want = tc.protein_tiles(long_reads, W, step)
    out = []
    for tiled in (True, False):
        with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0", "-y", "9"]) as s:
            if tiled:
                s.set_queries([x[1] for x in long_reads], [x[0] for x in long_reads], width=W, tile_step=step)
            else:
                s.set_queries([t[1] for t in want], [t[0] for t in want], width=W)
            s.run()
            out.append((s.output().split(b"\n"), s.query_tiles(), s.hits_rows()[0]["query_record"]))
    (got, tiles, qrec), (base, _, _) = out
    offsets = tiles["offset"][qrec].tolist()
    assert len(got) == len(base) and len(offsets) > 30 and max(offsets) > 0
    hit = -1
    for line, plain in zip(got, base):
        cols = plain.split(b"\t")
        if plain.startswith(b"# "):
            hit += 1
            cols[6], cols[7] = b"%d" % (int(cols[6]) + offsets[hit]), b"%d" % (int(cols[7]) + offsets[hit])
        elif plain.startswith(b"Query\t"):
            cols[1], cols[3] = b"%d" % (int(cols[1]) + offsets[hit]), b"%d" % (int(cols[3]) + offsets[hit])
        assert line == b"\t".join(cols)
    assert hit + 1 == len(offsets)


def test_search_cli_minus_t(dataset, long_reads, tmp_path):
    d = dataset("syn_small")
    W, step = 127, 64
    with open(tmp_path / "reads.fa", "w") as f:
        for name, seq in long_reads:
            f.write(f">{name}\n{seq}\n")
    with open(tmp_path / "tiles.fa", "w") as f:
        for t in tc.protein_tiles(long_reads, W, step, 300):
            f.write(f">{t[0]}\n{t[1]}\n")
    db = os.path.join(d, "db")
    for args, out in ((["-T", str(step), "-X", "300", str(tmp_path / "reads.fa")], "tiled.out"),
                      ([str(tmp_path / "tiles.fa")], "explicit.out")):
        r = subprocess.run([cases.GHOSTM, "search", "-w", str(W), "-d", db] + args + [str(tmp_path / out)],
                           capture_output=True)
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "tiled.out").read_bytes() == (tmp_path / "explicit.out").read_bytes()
    assert (tmp_path / "tiled.out").stat().st_size > 1000


@pytest.mark.parametrize("style", ["0", "1", "2"])
def test_search_equals_reference_on_explicit_tiles(dataset, tmp_path, style):
    """tests/golden/tiles_y*.out: the reference's `qry -l 32` + `aln` on the
    reads' tiles listed as records under repeated names
    (tests/golden/make_tiles_golden.py); `search -T 16` on the reads prints
    those bytes."""
    d = dataset("protein_testset")
    want = open(os.path.join(cases.GOLDEN, f"tiles_y{style}.out"), "rb").read()
    out = str(tmp_path / "got.out")
    r = subprocess.run([cases.GHOSTM, "search", "-w", "32", "-T", "16", "-y", style, "-d", os.path.join(d, "db"),
                        os.path.join(cases.GOLDEN, "tiles_reads.fasta"), out], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert len(want) > 2000 and open(out, "rb").read() == want


# ------------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_under_lds_poison(pattern, dataset):
    """The tiled kernels stage their letter and codon tables in LDS: the protein
    and DNA record cases on the poison build, one child process per pattern."""
    here = os.path.dirname(os.path.abspath(__file__))
    poison = os.path.join(os.path.dirname(here), "ghostm_amd", "lib", "libghostm_hip_poison.so")
    assert os.path.exists(poison), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=poison, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(here, "tiles_poison_child.py"), dataset("protein_testset")],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["sets"] == len(tc.PROTEIN_CASES) + len(tc.DNA_CASES)


# ------------------------------------------------------------------ refusals
def raw_call(s, seqs, names, width=127, dna=0, step=64, raw_len=None, offsets=None, lengths=None, null=None):
    lib = native.load()
    raw = np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)
    lens = np.array([len(x) for x in seqs] if lengths is None else lengths, dtype=np.uint32)
    offs = np.zeros(len(lens), dtype=np.uint64)
    if offsets is not None:
        offs[:] = offsets
    elif len(lens) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    name_buf = b"".join(x + b"\n" for x in names)
    args = [s._h, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            int(lens.sum()) if raw_len is None else raw_len,
            offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            name_buf, len(name_buf), len(lens), width, dna, 0, 0, step]
    if null is not None:
        args[null] = None
    return lib.GhostmSessionSetQueriesTiled(*args)


def test_refusals_leave_the_old_set(dataset, long_reads):
    d = dataset("syn_small")
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_queries([x[1] for x in long_reads], [x[0] for x in long_reads], width=127, tile_step=64)
        s.run()
        want = (s.output(), s.query_tiles().tobytes(), s.query_lengths().tolist())
        assert len(want[0]) > 0
        sets = s.stats()["query_sets"]

        def still_there(what):
            assert native.last_error(), what
            assert s.stats()["query_sets"] == sets, what
            assert (s.query_tiles().tobytes(), s.query_lengths().tolist()) == want[1:], what
            s.run()
            assert s.output() == want[0], what

        seqs, names = [b"MKVLAAGIVG" * 30, b"ACDEFGHIKL" * 20], [b"a", b"b"]
        for step, width in ((0, 127), (128, 127), (61, 60), (500, 500)):
            with pytest.raises(GhostmError, match="step"):
                s.set_queries(seqs, names, width=width, tile_step=step)
            still_there(f"step {step}")
        with pytest.raises(GhostmError, match="step"):
            s.set_queries_fasta(os.path.join(d, "q.fa"), width=100, tile_step=0)
        still_there("fasta step 0")
        with pytest.raises(GhostmError):
            s.set_queries_fasta(os.path.join(d, "missing.fa"), width=100, tile_step=5)
        still_there("fasta missing")
        for null in (1, 3, 4, 5):  # letters, offsets, lengths, names
            assert raw_call(s, seqs, names, null=null) != 0
            assert "null" in native.last_error()
            still_there(f"null argument {null}")
        assert raw_call(s, seqs, names, raw_len=400) != 0  # the second record ends past the buffer
        assert "outside the letter buffer" in native.last_error()
        still_there("record outside the buffer")
        assert raw_call(s, seqs, names, offsets=[0, 1 << 40]) != 0
        still_there("offset outside the buffer")
        # one record over the per-record limit of 1024 output records
        assert raw_call(s, [b"A" * (127 + 1024)], [b"a"], step=1) != 0
        assert "limit" in native.last_error()
        still_there("per-record limit")
        # 33100 records x 1024 tiles x 127 bytes wrap the chunk's 32-bit byte count (the records share their letters)
        n = 33100
        assert raw_call(s, [b"A" * (127 + 1023)], [b"a"] * n, step=1, offsets=[0] * n, lengths=[127 + 1023] * n,
                        raw_len=127 + 1023) != 0
        assert "32-bit" in native.last_error()
        still_there("chunk wrap")
        # a good set still replaces it
        s.set_queries(seqs, names, width=127, tile_step=64)
        assert s.stats()["query_sets"] == sets + 1 and len(s.query_tiles()) == 4 + 3
        # and an untiled one forgets the table
        s.set_queries(seqs, names, width=127)
        assert len(s.query_tiles()) == 0


def test_shard_session_refuses_a_tiled_set(dataset):
    d = dataset("syn_small")
    argv = ["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]
    with Session(argv, shard=(1, 2)) as s:
        s.run()
        want = (s.shard_range(), s.output())
        with pytest.raises(GhostmError, match="shard"):
            s.set_queries(["MKV" * 100], ["a"], width=127, tile_step=64)
        with pytest.raises(GhostmError, match="shard"):
            s.set_queries_fasta(os.path.join(d, "q.fa"), width=127, tile_step=64)
        s.run()  # its own queries are still there
        assert (s.shard_range(), s.output()) == want and len(want[1]) > 0
