"""Query sets replaced on a live session (GhostmSessionCreateDb,
GhostmSessionSetQueries*, `ghostm search`): FASTA in, the database stays
resident, the letters are coded / six-frame translated on the GPU straight into
the session's query chunks (qformat.hip, the kernels with the record lengths).

Every comparison is byte equality: the resident records against the .seq files
of the CPU formatter (`ghostm qry` without -D, pinned to the reference by
tests/test_formatter.py), the record lengths against last-non-X + 1 of those
bytes, and the searches against a session created on the formatted files."""
import os
import random
import subprocess

import numpy as np
import pytest

import cases
from ghostm_amd import GhostmError
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

AA = "ARNDCQEGHILKMFPSTWYV"


# ------------------------------------------------------------------ kernel level
@pytest.fixture(scope="module")
def db_session(dataset):
    d = dataset("protein_testset")
    with Session.for_db(["-d", os.path.join(d, "db"), "-D", "0"]) as s:
        yield s


def qry_chunks(prefix):
    """[(nseq, L, codes[nseq, L])] of the files `ghostm qry` wrote."""
    division = int(np.fromfile(prefix + ".inf", dtype="<i4", count=1)[0])
    out = []
    for c in range(division):
        n, width = (int(x) for x in np.fromfile(f"{prefix}_{c}.inf", dtype="<u4", count=2))
        out.append((n, width, np.fromfile(f"{prefix}_{c}.seq", dtype=np.uint8).reshape(n, width)))
    return out


def residues(codes):
    """WriteOutput's query length of every row: last non-X code + 1, at least 1."""
    nonx = codes != 23
    last = codes.shape[1] - np.argmax(nonx[:, ::-1], axis=1)
    return np.where(nonx.any(axis=1), last, 1).astype(np.uint32)


def check_against_qry(s, fa, tmp_path, width, dna, chunk_mb=0):
    opts = ["-l", str(width)] + (["-t", "d"] if dna else []) + (["-L", str(chunk_mb)] if chunk_mb else [])
    r = subprocess.run([cases.GHOSTM, "qry", "-i", str(fa), "-o", str(tmp_path / "q")] + opts, check=True,
                       capture_output=True)
    cut = s.set_queries_fasta(str(fa), width=width, dna=dna, chunk_mb=chunk_mb)
    assert cut == r.stderr.count(b"warning : the length of sequence is over.")
    chunks = qry_chunks(str(tmp_path / "q"))
    want_len = []
    for c, (n, w, codes) in enumerate(chunks):
        got = s.query_records(c)
        assert got.size == n * w, f"chunk {c}"
        assert got.tobytes() == codes.tobytes(), f"chunk {c}"
        want_len.append(residues(codes))
    with pytest.raises(GhostmError):
        s.query_records(len(chunks))
    got_len = s.query_lengths()
    assert got_len.tolist() == (np.concatenate(want_len).tolist() if want_len else [])
    return chunks


def protein_fasta(width, r):
    rand = lambda n: "".join(r.choice(AA) for _ in range(n))  # noqa: E731
    lens = []
    for n in (1, 0, width - 1, width, width + 1):
        if n >= 0 and n not in lens:
            lens.append(n)
    recs = [(f"len{n}", rand(n)) for n in lens]
    recs += [("only_x", "XXX"), ("ends_in_x", "MK" + "xUO"), ("lower_unknown", "acdefBZJ*u1-wy"),
             ("tail_x_long", rand(max(width - 3, 1)) + "XXXXXX"), ("last", rand(width // 2 + 1))]
    return recs


def write_fasta(path, recs):
    with open(path, "w") as f:
        for name, seq in recs:
            f.write(f">{name}\n" + (seq + "\n" if seq else ""))


@pytest.mark.parametrize("width_opt,width", [(1, 1), (63, 63), (64, 64), (65, 65), (300, 127)])
def test_protein_records_and_lengths(db_session, tmp_path, width_opt, width):
    recs = protein_fasta(width, random.Random(width))
    write_fasta(tmp_path / "p.fa", recs)
    chunks = check_against_qry(db_session, tmp_path / "p.fa", tmp_path, width_opt, False)
    assert [(n, w) for n, w, _ in chunks] == [(len(recs), width)]
    assert db_session.query_lengths()[[k for k, (n, _) in enumerate(recs) if n == "only_x"][0]] == 1


@pytest.mark.parametrize("n", [1, 5])
def test_protein_record_counts(db_session, tmp_path, n):
    """One record, and a count that is no multiple of the waves per block."""
    recs = protein_fasta(64, random.Random(n))[2:2 + n]
    write_fasta(tmp_path / "p.fa", recs)
    chunks = check_against_qry(db_session, tmp_path / "p.fa", tmp_path, 64, False)
    assert chunks[0][0] == n


def dna_fasta(first, r):
    rand = lambda n: "".join(r.choice("ACGT") for _ in range(n))  # noqa: E731
    # frame 0: TAA is letter 63 (the last of the first 64-letter group), the ATG
    # that clears it letter 64
    stop_then_atg = "GCT" * 63 + "TAA" + "ATG" + "GCT" * 70
    # TTA: a stop (TAA) on the reverse strand only
    reverse_stop = "CCG" * 20 + "TTA" + "CCG" * 110
    with_n = list(rand(first + 3))
    for k in range(0, len(with_n), 7):
        with_n[k] = "N"
    return [("first", rand(first)), ("shorter", rand(first // 2)), ("longer", rand(first + 7)),
            ("with_n", "".join(with_n)), ("stop_then_atg", stop_then_atg), ("reverse_stop", reverse_stop),
            ("lower_gap", "atg-ry" + rand(first).lower()), ("stops", "TAATAGTGA" * 43), ("empty", "")]


@pytest.mark.parametrize("first", [1, 2, 3, 5, 191, 192, 193, 381])
def test_dna_frames_and_lengths(db_session, tmp_path, first):
    recs = dna_fasta(first, random.Random(first))
    write_fasta(tmp_path / "d.fa", recs)
    chunks = check_against_qry(db_session, tmp_path / "d.fa", tmp_path, 381, True)
    assert [(n, w) for n, w, _ in chunks] == [(6 * len(recs), 127)]


def test_dna_stop_cleared_across_groups(db_session, tmp_path):
    """The crafted read as the chunk's first (its whole length kept): frame 0 is
    A x 63, then the stop, then M and A again."""
    recs = dna_fasta(381, random.Random(0))
    recs = [recs[4]] + recs[:4]
    write_fasta(tmp_path / "d.fa", recs)
    chunks = check_against_qry(db_session, tmp_path / "d.fa", tmp_path, 600, True)
    frame0 = chunks[0][2][0]
    assert frame0[:63].tolist() == [0] * 63 and frame0[63] == 24 and frame0[64] == 12 and frame0[65] == 0


def test_several_chunks_of_letters(db_session, tmp_path):
    """-L 1: the FASTA's records over more than one resident chunk."""
    r = random.Random(8)
    recs = [(f"q{i}", "".join(r.choice(AA) for _ in range(r.randint(900, 1100)))) for i in range(2300)]
    write_fasta(tmp_path / "p.fa", recs)
    chunks = check_against_qry(db_session, tmp_path / "p.fa", tmp_path, 100, False, chunk_mb=1)
    assert len(chunks) == 3


# ------------------------------------------------------------------ session level
def qry_params(name, d):
    _, args = [t for t in cases.DATASETS[name] if t[0] == "qry"][0]
    a = [x.format(d=d, golden=cases.GOLDEN) for x in args]
    opt = lambda flag, default: a[a.index(flag) + 1] if flag in a else default  # noqa: E731
    return dict(path=opt("-i", None), width=int(opt("-l", "75")), dna=opt("-t", "p") == "d",
                chunk_mb=int(opt("-L", "0")))


_FILE_RESULTS = {}


def file_session_results(d, opts, tag):
    """output, hits (and for -y 7 the paths) of a session on the formatted files, once."""
    key = (d, tuple(opts))
    if key not in _FILE_RESULTS:
        with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]
                     + list(opts)) as s:
            s.run()
            res = [s.output(), s.hits()]
            if tag == "path":
                res += list(s.hits_path())
            _FILE_RESULTS[key] = res
    return _FILE_RESULTS[key]


SESSION_CASES = [
    ("protein_testset", []),
    ("syn_small", []),
    ("syn_short", []),
    ("syn_dna", []),
    ("syn_chunks", []),
    ("syn_small", ["-y", "2", "-b", "20"]),
    ("syn_dna", ["-y", "6"]),
    ("syn_dna", ["-y", "7"]),
]


@pytest.mark.parametrize("name,opts", SESSION_CASES, ids=[f"{n}/{'_'.join(o) or 'default'}" for n, o in SESSION_CASES])
def test_db_session_equals_file_session(name, opts, dataset):
    d = dataset(name)
    tag = "path" if opts[:2] == ["-y", "7"] else ""
    want = file_session_results(d, opts, tag)
    p = qry_params(name, d)
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"] + list(opts)) as s:
        s.run()  # before any query set: nothing
        assert s.output() == b"" and len(s.hits()) == 0 and s.hit_capacity() == 0
        s.set_queries_fasta(**p)
        s.run()
        assert s.output() == want[0]
        assert s.hits().tobytes() == want[1].tobytes()
        if tag == "path":
            rec, ops = s.hits_path()
            assert rec.tobytes() == want[2].tobytes() and ops.tobytes() == want[3].tobytes()
        st = s.stats()
        assert st["query_sets"] == 1 and st["query_format_launches"] >= 1 and st["seconds_query_format"] > 0
        assert st["seconds_query_read"] > 0 and st["seconds_query_load"] > 0
        assert st["queries"] == len(s.query_lengths())
    with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as f:
        # the accessors on a file-loaded session: the .seq files' own bytes
        for c, (n, w, codes) in enumerate(qry_chunks(os.path.join(d, "q"))):
            assert f.query_records(c).tobytes() == codes.tobytes()
            if c == 0:
                assert f.query_lengths()[:n].tolist() == residues(codes).tolist()
        assert f.stats()["query_sets"] == 0


def read_fasta(path):
    recs = []
    for line in open(path):
        line = line.rstrip("\r\n")
        if line.startswith(">"):
            recs.append([line[1:].lstrip("> "), ""])
        elif recs and line:
            recs[-1][1] += line
    return recs


def test_reuse_and_set_queries_from_records(dataset, tmp_path):
    """One database session: set A, run; set B, run; set A again, run. Then the
    same from records in memory (set_queries) and on a file-created session."""
    d = dataset("readme_kat")
    db = os.path.join(d, "db")
    fa_a = os.path.join(cases.GOLDEN, "testset_db.fasta")       # readme_kat's queries: qry -t d
    fa_b = os.path.join(cases.GOLDEN, "testset_queries.fasta")  # proteins, -l 60
    subprocess.run([cases.GHOSTM, "qry", "-i", fa_b, "-o", str(tmp_path / "qb"), "-l", "60"], check=True,
                   capture_output=True)
    want_a = file_session_results(d, [], "")
    with Session(["-i", str(tmp_path / "qb"), "-d", db, "-o", os.devnull, "-D", "0"]) as f:
        f.run()
        want_b = [f.output(), f.hits()]
        assert len(want_b[1]) > 0
        # a file-created session takes a new set too
        f.set_queries_fasta(fa_a, dna=True)
        f.run()
        assert f.output() == want_a[0] and f.hits().tobytes() == want_a[1].tobytes()
    with Session.for_db(["-d", db, "-o", os.devnull, "-D", "0"]) as s:
        s.set_queries_fasta(fa_a, dna=True)
        s.run()
        first = (s.output(), s.hits().tobytes())
        assert len(first[0]) > 0
        s.set_queries_fasta(fa_b, width=60)
        assert s.output() == b"" and len(s.hits()) == 0  # the last run's results are dropped
        s.run()
        assert s.output() == want_b[0] and s.hits().tobytes() == want_b[1].tobytes()
        s.set_queries_fasta(fa_a, dna=True)
        s.run()
        assert (s.output(), s.hits().tobytes()) == first == (want_a[0], want_a[1].tobytes())
        assert s.stats()["query_sets"] == 3
        records_a = [s.query_records(0).tobytes(), s.query_lengths().tolist()]
        # the same records from memory
        recs = read_fasta(fa_a)
        s.set_queries([x[1] for x in recs], [x[0] for x in recs], dna=True)
        assert [s.query_records(0).tobytes(), s.query_lengths().tolist()] == records_a
        s.run()
        assert (s.output(), s.hits().tobytes()) == first
        recs = read_fasta(fa_b)
        s.set_queries([x[1].encode() for x in recs], [x[0].encode() for x in recs], width=60)
        s.run()
        assert s.output() == want_b[0] and s.hits().tobytes() == want_b[1].tobytes()
        assert s.stats()["query_sets"] == 5
        # a file that cannot be opened is refused and the session stays as it was
        with pytest.raises(GhostmError):
            s.set_queries_fasta(str(tmp_path / "missing.fa"))
        assert s.stats()["query_sets"] == 5
        s.run()
        assert s.output() == want_b[0]


def test_set_output_and_run_to_file(dataset, tmp_path):
    d = dataset("protein_testset")
    want = file_session_results(d, [], "")
    with Session.for_db(["-d", os.path.join(d, "db"), "-D", "0"]) as s:
        s.set_queries_fasta(**qry_params("protein_testset", d))
        s.set_output(str(tmp_path / "a.out"))
        s.run(to_file=True)
        s.set_output(str(tmp_path / "b.out"))
        s.write()
        assert (tmp_path / "a.out").read_bytes() == want[0] == (tmp_path / "b.out").read_bytes()


@pytest.mark.parametrize("opts", [[], ["-y", "6"], ["-y", "7"]], ids=["y0", "y6", "y7"])
def test_search_cli_equals_qry_plus_aln(dataset, tmp_path, opts):
    d = dataset("protein_testset")
    db = os.path.join(d, "db")
    fas = [os.path.join(cases.GOLDEN, "testset_queries.fasta"), os.path.join(dataset("syn_small"), "q.fa")]
    want, warned = [], 0
    for k, fa in enumerate(fas):
        q = str(tmp_path / f"q{k}")
        r = subprocess.run([cases.GHOSTM, "qry", "-i", fa, "-o", q, "-l", "60"], check=True, capture_output=True)
        warned += r.stderr.count(b"warning : the length of sequence is over.")
        out = str(tmp_path / f"want{k}.out")
        subprocess.run([cases.GHOSTM, "aln", "-i", q, "-d", db, "-o", out] + opts, check=True, capture_output=True)
        want.append(open(out, "rb").read())
    assert len(want[0]) > 0 and warned > 0
    outs = [str(tmp_path / f"got{k}.out") for k in range(2)]
    r = subprocess.run([cases.GHOSTM, "search", "-w", "60", "-d", db] + opts + [fas[0], outs[0], fas[1], outs[1]],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count(b"warning : the length of sequence is over.") == warned
    for k in range(2):
        assert open(outs[k], "rb").read() == want[k]


def test_shard_session_refuses_a_new_set(dataset):
    d = dataset("syn_small")
    argv = ["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]
    with Session(argv, shard=(1, 2)) as ref:
        ref.run()
        want = (ref.shard_range(), ref.output())
    assert len(want[1]) > 0
    with Session(argv, shard=(1, 2)) as s:
        with pytest.raises(GhostmError, match="shard"):
            s.set_queries_fasta(**qry_params("syn_small", d))
        with pytest.raises(GhostmError, match="shard"):
            s.set_queries(["MKV"], ["a"])
        s.run()  # its own queries are still there
        assert (s.shard_range(), s.output()) == want
