"""Databases replaced on a live session (GhostmSessionCreateQueries,
GhostmSessionSetDb*, `ghostm search -f`): FASTA in, the letters coded on the GPU
straight into the session's DB chunks (kernels.h k_db_code) and the k-mer index
built there from the device residues (index.hip), no files.

Every comparison is byte equality: the resident residues, index and headers
against the .seq, .ind, .inf and .pos files of the CPU formatter (`ghostm db`
without -D, pinned to the reference by tests/test_formatter.py), and the
searches against a session created on the formatted files."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cases
import setdb_cases as sd
from ghostm_amd import GhostmError, native
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POISON_LIB = os.path.join(os.path.dirname(HERE), "ghostm_amd", "lib", "libghostm_hip_poison.so")


# ------------------------------------------------------------------ kernel level
@pytest.fixture(scope="module")
def bare():
    """A session with neither input: the database comes from set_db*."""
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "1"]) as s:
        yield s


# every chunk length at k = 3 and 4; k = 5 (a 134 MB keys_count) either side of the lane and the workgroup width
BYTES_K = [(n, k) for n in sd.CHUNK_BYTES for k in (3, 4)] + [(n, 5) for n in (16, 17, 4096, 4097)]


@pytest.mark.parametrize("nbytes,k", BYTES_K, ids=[f"{n}B-k{k}" for n, k in BYTES_K])
def test_chunk_lengths(bare, tmp_path, nbytes, k):
    recs = sd.records_of_bytes(nbytes, random.Random(nbytes * 8 + k))
    sd.write_fasta(tmp_path / "db.fa", recs)
    want = sd.check_fasta(bare, tmp_path / "db.fa", tmp_path / "db", k=k)
    assert [(w["nseq"], w["len"]) for w in want] == [(len(recs), nbytes)]


@pytest.mark.parametrize("k", [3, 4, 5])
def test_subject_lengths_letters_and_x_windows(bare, tmp_path, k):
    recs = sd.edge_records(k, random.Random(k))
    sd.write_fasta(tmp_path / "db.fa", recs)
    want = sd.check_fasta(bare, tmp_path / "db.fa", tmp_path / "db", k=k)[0]
    # the fixture does what it says: a subject of exactly `span` residues has no
    # key, one of span + 1 has two windows; an X anywhere in the span drops the window
    starts = dict(zip([n for n, _ in recs], want["starts"].tolist()))
    pos = set(want["pos"].tolist())
    assert starts[f"len{k}"] not in pos and starts["just_span_again"] not in pos
    assert {starts[f"len{k + 1}"], starts[f"len{k + 1}"] + 1} <= pos
    for t in range(k):
        a = starts[f"x_at{t}"]
        hit = {a + 10 + t - j for j in range(k)}  # the windows that hold the X
        assert not (hit & pos) and a + 10 + t + 1 in pos and a + 10 + t - k in pos
    codes = want["seq"]
    a = starts["unknown"]
    assert codes[a + k + 1] == 23 and codes[a + k + 2] == 23  # U, O
    assert want["seq"][0] == 25 and want["seq"][-1] == 25 and want["seq"][-2] == 25  # empty first and last


@pytest.mark.parametrize("recs", [[("only", "MKVLAAGIWQRTSPL")], [("only_empty", "")], [("a", ""), ("b", "")]],
                         ids=["one_record", "one_empty_record", "two_empty_records"])
def test_single_records(bare, tmp_path, recs):
    sd.write_fasta(tmp_path / "db.fa", recs)
    want = sd.check_fasta(bare, tmp_path / "db.fa", tmp_path / "db", k=4)
    assert [w["nseq"] for w in want] == [len(recs)]


def test_three_chunks(bare, dataset):
    """syn_chunks' db.fa with chunk_mb=1: the chunk count and every chunk's
    arrays equal the dataset's own files (`ghostm db -l 1`)."""
    d = dataset("syn_chunks")
    want = sd.db_files(os.path.join(d, "db"))
    assert len(want) == 3
    bare.set_db_fasta(os.path.join(d, "db.fa"), chunk_mb=1)
    sd.assert_resident_equals_files(bare, want)
    st = bare.stats()
    assert st["db_format_launches"] == 3 and st["seconds_db_format"] > st["seconds_db_code"] > 0
    assert st["seconds_db_read"] > 0 and st["seconds_db_load"] > 0


def test_accessors_on_a_file_session(dataset):
    """db_chunks / db_records / db_index of a database loaded from files: the
    files' own bytes; and the default path formats nothing."""
    d = dataset("syn_short")
    want = sd.db_files(os.path.join(d, "db"))
    with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0", "-y", "1"]) as s:
        sd.assert_resident_equals_files(s, want)
        st = s.stats()
        assert st["db_sets"] == 0 and st["db_format_launches"] == 0 and st["seconds_db_format"] == 0
        with pytest.raises(GhostmError):
            s.db_records(len(want))
        with pytest.raises(GhostmError):
            s.db_index(len(want))
    with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        s.run()
        st = s.stats()
        assert st["db_sets"] == 0 and st["db_format_launches"] == 0 and st["seconds_db_load"] == 0


# ------------------------------------------------------------------ search level
def tool_params(name, d, tool):
    _, args = [t for t in cases.DATASETS[name] if t[0] == tool][0]
    a = [x.format(d=d, golden=cases.GOLDEN) for x in args]
    return lambda flag, default: a[a.index(flag) + 1] if flag in a else default


def db_params(name, d):
    opt = tool_params(name, d, "db")
    return dict(path=opt("-i", None), k=int(opt("-k", "4")), chunk_mb=int(opt("-l", "0")))


def qry_params(name, d):
    opt = tool_params(name, d, "qry")
    return dict(path=opt("-i", None), width=int(opt("-l", "75")), dna=opt("-t", "p") == "d",
                chunk_mb=int(opt("-L", "0")))


_FILE_RESULTS = {}


def file_session_results(d, opts):
    """(output, hits, stats) of a session on the formatted files, once."""
    key = (d, tuple(opts))
    if key not in _FILE_RESULTS:
        with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]
                     + list(opts)) as s:
            s.run()
            _FILE_RESULTS[key] = (s.output(), s.hits(), s.stats())
    return _FILE_RESULTS[key]


SEARCH_CASES = [
    ("protein_testset", []),
    ("syn_small", []),
    ("syn_small", ["-y", "2"]),
    ("syn_small", ["-y", "7"]),
    ("syn_small", ["-y", "10"]),
    ("syn_dna", []),
    ("syn_short", []),
    ("syn_chunks", []),
    ("syn_chunks", ["-b", "20", "-y", "2"]),
    ("cfg2_single", []),
    ("syn_repeat", []),
    ("syn_subj10", []),
    ("syn_subj4", []),
]
SEARCH_IDS = [f"{n}/{'_'.join(o) or 'default'}" for n, o in SEARCH_CASES]


def assert_same_search(s, want, name):
    s.run()
    assert s.output() == want[0]
    assert s.hits().tobytes() == want[1].tobytes()
    assert len(want[1]) > 0
    st = s.stats()
    # the K2 restart levels are chosen from end_gap: the same launches as on the files
    assert st["score_launches_levels"] == want[2]["score_launches_levels"], name
    assert st["candidates"] == want[2]["candidates"]
    return st


@pytest.mark.parametrize("name,opts", SEARCH_CASES, ids=SEARCH_IDS)
def test_queries_from_files_db_from_fasta(name, opts, dataset):
    """for_queries(-i q) + set_db_fasta against the session on the files."""
    d = dataset(name)
    want = file_session_results(d, opts)
    with Session.for_queries(["-i", os.path.join(d, "q"), "-o", os.devnull, "-D", "0"] + list(opts)) as s:
        s.run()  # before any database: nothing
        assert s.output() == b"" and len(s.hits()) == 0 and s.db_chunks() == []
        s.set_db_fasta(**db_params(name, d))
        st = assert_same_search(s, want, name)
        assert st["db_sets"] == 1 and st["db_format_launches"] == len(s.db_chunks()) >= 1
        assert st["seconds_db_format"] > st["seconds_db_code"] > 0
        assert st["query_sets"] == 0


@pytest.mark.parametrize("name,opts", SEARCH_CASES, ids=SEARCH_IDS)
def test_both_inputs_from_fasta(name, opts, dataset):
    """A bare session + set_db_fasta + set_queries_fasta: no formatted file read."""
    d = dataset(name)
    want = file_session_results(d, opts)
    with Session.for_queries(["-o", os.devnull, "-D", "0"] + list(opts)) as s:
        s.set_db_fasta(**db_params(name, d))
        s.run()  # no queries yet: nothing
        assert s.output() == b"" and len(s.hits()) == 0
        s.set_queries_fasta(**qry_params(name, d))
        st = assert_same_search(s, want, name)
        assert st["db_sets"] == 1 and st["query_sets"] == 1


def test_levels_cases_do_run_the_level_kernel(dataset):
    """The end_gap check above is not vacuous: syn_subj10 launches the restart-level K2."""
    assert file_session_results(dataset("syn_subj10"), [])[2]["score_launches_levels"] > 0


# ------------------------------------------------------------------ swap
@pytest.fixture(scope="module")
def swap_data(dataset, tmp_path_factory):
    """syn_small's database A, the first half of its records as database B, and
    the file sessions' -y 0 results on each."""
    d = dataset("syn_small")
    tmp = tmp_path_factory.mktemp("swap")
    recs = sd.read_fasta(os.path.join(d, "db.fa"))
    half = recs[: len(recs) // 2]
    sd.write_fasta(tmp / "b.fa", half)
    sd.format_db(tmp / "b.fa", tmp / "b")
    want_a = file_session_results(d, [])
    with Session(["-i", os.path.join(d, "q"), "-d", str(tmp / "b"), "-o", os.devnull, "-D", "0"]) as s:
        s.run()
        want_b = (s.output(), s.hits(), s.stats())
    assert len(want_b[1]) > 0 and want_b[0] != want_a[0]
    return dict(d=d, fa_a=os.path.join(d, "db.fa"), fa_b=str(tmp / "b.fa"), recs=recs, half=half, want_a=want_a,
                want_b=want_b)


def test_swap_a_b_a(swap_data):
    """A, then B (the same hits at the same scores in another search space),
    then A again on one session: a stale E-value cache, subject table or chunk
    base shows as a differing line."""
    w = swap_data
    # the same hit at the same score prints another E-value on B: the case is there
    ha, hb = w["want_a"][1], w["want_b"][1]
    both = set(zip(ha["query_id"].tolist(), ha["db_id"].tolist(), ha["score"].tolist())) & set(
        zip(hb["query_id"].tolist(), hb["db_id"].tolist(), hb["score"].tolist()))
    assert both
    with Session.for_queries(["-i", os.path.join(w["d"], "q"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_db_fasta(w["fa_a"])
        s.run()
        run1 = (s.output(), s.hits().tobytes())
        assert run1 == (w["want_a"][0], w["want_a"][1].tobytes())
        s.set_db_fasta(w["fa_b"])
        assert s.output() == b"" and len(s.hits()) == 0  # the last run's results are dropped
        s.run()
        assert (s.output(), s.hits().tobytes()) == (w["want_b"][0], w["want_b"][1].tobytes())
        s.set_db_fasta(w["fa_a"])
        s.run()
        assert (s.output(), s.hits().tobytes()) == run1
        assert s.stats()["db_sets"] == 3


def test_set_db_from_records_equals_fasta(swap_data, tmp_path):
    w = swap_data
    with Session.for_queries(["-i", os.path.join(w["d"], "q"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_db_fasta(w["fa_b"])
        fasta = (s.db_chunks(), s.db_records(0).tobytes(), [x.tobytes() for x in s.db_index(0)[1:]])
        s.set_db([x[1] for x in w["half"]], [x[0] for x in w["half"]])
        assert (s.db_chunks(), s.db_records(0).tobytes(), [x.tobytes() for x in s.db_index(0)[1:]]) == fasta
        s.run()
        assert (s.output(), s.hits().tobytes()) == (w["want_b"][0], w["want_b"][1].tobytes())
        s.set_db([x[1].encode() for x in w["recs"]], [x[0].encode() for x in w["recs"]], k=4, chunk_mb=0)
        s.run()
        assert (s.output(), s.hits().tobytes()) == (w["want_a"][0], w["want_a"][1].tobytes())
        assert s.stats()["db_sets"] == 3 and s.stats()["seconds_db_read"] == 0
        # a newline among the letters of a record given in memory is one more unknown letter
        s.set_db(["MKV\nLA", "WWW"], ["a", "b"])
        sd.write_fasta(tmp_path / "x.fa", [("a", "MKVXLA"), ("b", "WWW")])
        assert s.db_records(0).tobytes() == sd.format_db(tmp_path / "x.fa", tmp_path / "x")[0]["seq"].tobytes()


def test_file_session_takes_a_new_database(swap_data):
    w = swap_data
    d = w["d"]
    with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        s.run()
        assert s.output() == w["want_a"][0] and s.stats()["db_sets"] == 0
        s.set_db_fasta(w["fa_b"])
        s.run()
        assert (s.output(), s.hits().tobytes()) == (w["want_b"][0], w["want_b"][1].tobytes())
        assert s.stats()["db_sets"] == 1
        s.set_db_fasta(w["fa_a"])
        s.run()
        assert (s.output(), s.hits().tobytes()) == (w["want_a"][0], w["want_a"][1].tobytes())


def test_equal_second_set_allocates_nothing(swap_data):
    """The old chunks' blocks go to the pool and the next set of the same size
    takes every one of them back: the pool holds the same bytes after each set
    (a block allocated anew would leave its predecessor cached)."""
    w = swap_data
    with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
        s.set_db_fasta(w["fa_a"])
        first = native.device_pool_info()[0]
        for _ in range(2):
            s.set_db_fasta(w["fa_a"])
            assert native.device_pool_info()[0] == first
        assert s.stats()["db_sets"] == 3


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_session_as_it_was(swap_data, tmp_path):
    w = swap_data
    with Session.for_queries(["-i", os.path.join(w["d"], "q"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_db_fasta(w["fa_b"])
        s.run()
        before = (s.output(), s.db_chunks(), s.db_records(0).tobytes())
        assert before[0] == w["want_b"][0]
        lib = native.load()
        u8p, u32p, u64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
        raw = np.frombuffer(b"MKVLAW", dtype=np.uint8)
        off = np.array([0, 3], dtype=np.uint64)
        ln = np.array([3, 3], dtype=np.uint32)
        args = lambda **kw: [  # noqa: E731
            s._h, kw.get("raw", raw.ctypes.data_as(u8p)), 6, kw.get("off", off.ctypes.data_as(u64p)),
            kw.get("ln", ln.ctypes.data_as(u32p)), kw.get("names", b"a\nb\n"), 4, 2, kw.get("k", 4), kw.get("mb", 0)]
        refused = [
            lambda: lib.GhostmSessionSetDb(*args(raw=None)),
            lambda: lib.GhostmSessionSetDb(*args(off=None)),
            lambda: lib.GhostmSessionSetDb(*args(ln=None)),
            lambda: lib.GhostmSessionSetDb(*args(names=None)),
            lambda: lib.GhostmSessionSetDbFasta(s._h, None, 4, 0),
            # a record outside the letter buffer
            lambda: lib.GhostmSessionSetDb(*args(ln=np.array([3, 4], dtype=np.uint32).ctypes.data_as(u32p))),
            lambda: lib.GhostmSessionSetDb(*args(off=np.array([0, 7], dtype=np.uint64).ctypes.data_as(u64p))),
            lambda: lib.GhostmSessionSetDbFasta(s._h, str(tmp_path / "missing.fa").encode(), 4, 0),
            lambda: lib.GhostmSessionSetDbFasta(s._h, w["fa_a"].encode(), 0, 0),      # k = 0
            lambda: lib.GhostmSessionSetDbFasta(s._h, w["fa_a"].encode(), 7, 0),      # weight 7
            lambda: lib.GhostmSessionSetDb(*args(k=0)),
            lambda: lib.GhostmSessionSetDb(*args(k=7)),
            lambda: lib.GhostmSessionSetDbFasta(s._h, w["fa_a"].encode(), 4, 2048),   # chunk_mb
            lambda: lib.GhostmSessionSetDb(*args(mb=2048)),
        ]
        for k, call in enumerate(refused):
            assert call() != 0, k
            assert native.last_error(), k
        # records in memory: one over the chunk limit is found by the cut, before anything is dropped
        with pytest.raises(GhostmError, match="too small max length"):
            s.set_db(["MKV", "A" * (1 << 20)], ["a", "b"], chunk_mb=1)
        assert s.stats()["db_sets"] == 1
        assert (s.db_chunks(), s.db_records(0).tobytes()) == before[1:]
        s.run()
        assert s.output() == before[0]


def test_shard_session_refuses_a_new_database(dataset):
    d = dataset("syn_small")
    argv = ["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]
    with Session(argv, shard=(1, 2)) as ref:
        ref.run()
        want = (ref.shard_range(), ref.output())
    assert len(want[1]) > 0
    with Session(argv, shard=(1, 2)) as s:
        with pytest.raises(GhostmError, match="shard"):
            s.set_db_fasta(os.path.join(d, "db.fa"))
        with pytest.raises(GhostmError, match="shard"):
            s.set_db(["MKV"], ["a"])
        assert len(s.db_chunks()) == 1
        s.run()  # its own database is still there
        assert (s.shard_range(), s.output()) == want


def test_fasta_record_over_the_chunk_limit_leaves_no_database(swap_data, tmp_path):
    """From a file the record is met only while the chunks load: the call
    raises and the session holds no database."""
    w = swap_data
    recs = [("ok", "MKVLAAGIWQRTSPL" * 4), ("big", "A" * (1 << 20)), ("after", "WWWWW")]
    sd.write_fasta(tmp_path / "big.fa", recs)
    with Session.for_queries(["-i", os.path.join(w["d"], "q"), "-o", os.devnull, "-D", "0"]) as s:
        s.set_db_fasta(w["fa_b"])
        s.run()
        assert len(s.hits()) > 0
        with pytest.raises(GhostmError, match="too small max length"):
            s.set_db_fasta(str(tmp_path / "big.fa"), chunk_mb=1)
        assert s.db_chunks() == []
        s.run()
        assert s.output() == b"" and len(s.hits()) == 0
        s.set_db_fasta(w["fa_b"])  # and it takes the next one
        s.run()
        assert s.output() == w["want_b"][0]


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("name,db_opts,search_opts", [("syn_short", ["-k", "3"], ["-k", "3"]),
                                                      ("syn_chunks", ["-l", "1"], ["-m", "1"])],
                         ids=["syn_short-k3", "syn_chunks-m1"])
def test_search_cli_from_fasta_equals_db_qry_aln(dataset, tmp_path, name, db_opts, search_opts):
    d = dataset(name)
    q = qry_params(name, d)
    db, qp, want = str(tmp_path / "db"), str(tmp_path / "q"), str(tmp_path / "want.out")
    fa = os.path.join(d, "db.fa")
    subprocess.run([cases.GHOSTM, "db", "-i", fa, "-o", db] + db_opts, check=True, capture_output=True)
    subprocess.run([cases.GHOSTM, "qry", "-i", q["path"], "-o", qp, "-l", str(q["width"])]
                   + (["-L", str(q["chunk_mb"])] if q["chunk_mb"] else []), check=True, capture_output=True)
    subprocess.run([cases.GHOSTM, "aln", "-i", qp, "-d", db, "-o", want], check=True, capture_output=True)
    got = str(tmp_path / "got.out")
    r = subprocess.run([cases.GHOSTM, "search", "-f", fa, "-w", str(q["width"])] + search_opts
                       + (["-c", str(q["chunk_mb"])] if q["chunk_mb"] else []) + [q["path"], got], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(want) > 0
    assert open(got, "rb").read() == open(want, "rb").read()


def test_search_cli_usage(tmp_path, dataset):
    d = dataset("syn_short")
    fa, q = os.path.join(d, "db.fa"), os.path.join(d, "q.fa")
    r = subprocess.run([cases.GHOSTM, "search", "-f", fa, "-d", os.path.join(d, "db"), q, str(tmp_path / "o")],
                       capture_output=True)
    assert r.returncode == 1 and not (tmp_path / "o").exists()
    r = subprocess.run([cases.GHOSTM, "search", q, str(tmp_path / "o")], capture_output=True)
    assert r.returncode == 1 and not (tmp_path / "o").exists()


# ------------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_under_lds_poison(pattern, dataset, tmp_path):
    """The coding kernel stages its table in LDS and the index kernels scan and
    rank there: the kernel-level edge set and syn_small's search on the poison
    build, one child process per pattern."""
    assert os.path.exists(POISON_LIB), "build the poison library (make -C ghostm_amd/csrc)"
    d = dataset("syn_small")
    env = dict(os.environ, GHOSTM_LIB_PATH=POISON_LIB, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(HERE, "setdb_poison_child.py"), d, str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["databases"] == len(sd.CHUNK_BYTES) + 2 and res["hits"] > 0
