"""Quality trimming and masking of FASTQ reads on the GPU (k_qual_trim,
ghostm_amd/csrc/read_quality.hip; QualityTrimGpu, GhostmSessionSetQuality,
GhostmSessionSetQueriesFastq*Tiled, `ghostm search -Q`).

Stage level: quality_trim against quality_trim_host and the Python model of
qual_cases.py, letters and records, on every case set and named case; the
counters move by the model's sums; a launch with more reads than waves; reads
over one upload piece; every refusal before any launch. Session level: letters
and qualities through set_queries(..., quals=...) on a DNA tiled set give the
model's records and the query records of the model's trimmed and masked letters.
End to end on the golden testset (the readme's database, testset_queries.fasta,
and its DNA reads, testset_db.fasta): a FASTQ of the golden reads, half of them
with a low-quality tail that is the back-translation of another subject, so the
untrimmed read hits a subject the trimmed read does not.

k_qual_trim uses no LDS (its header comment says so), so there is no run under
the LDS-poison build."""
import os
import random
import subprocess

import numpy as np
import pytest

import cases
import qual_cases as qc
import tile_cases as tc
from ghostm_amd import GhostmError, native, quality_trim, quality_trim_host, stage_qual_stats
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

COUNTERS = ("launches", "reads", "letters", "trimmed5", "trimmed3", "masked", "failed", "bad")


def check_stage(reads, params, launches=1):
    letters, qual, offs, lens = qc.lay_out(reads)
    want, want_out, sums = qc.model(letters, qual, offs, lens, params)
    before = stage_qual_stats()
    got, out = quality_trim(letters, qual, offs, lens, *params)
    after = stage_qual_stats()
    host, host_out = quality_trim_host(letters, qual, offs, lens, *params)
    assert out.tolist() == host_out.tolist() == want_out.tolist()
    assert got == host == want and qc.gaps_untouched(got, offs, lens)
    delta = {k: after[k] - before[k] for k in COUNTERS}
    on = any(params) and len(reads) > 0
    assert delta["launches"] == (launches if on else 0)
    for k in COUNTERS[1:]:
        assert delta[k] == (sums[k] if on else 0), k
    assert after["seconds_quality"] > before["seconds_quality"] or not on
    return out


# ------------------------------------------------------------------ stage level
@pytest.mark.parametrize("params", qc.PARAM_SETS)
def test_stage_equals_host_and_model(params):
    check_stage(qc.random_set(params)[0], params)


@pytest.mark.parametrize("name", sorted(qc.carry_cases()))
def test_named_cases(name):
    reads, params, check = qc.carry_cases()[name]
    check(check_stage(reads, params))


def test_more_reads_than_waves():
    reads = qc.grid_stride_set()
    assert len(reads) > 4 * 1024  # kQualBlocksMax blocks of four waves
    out = check_stage(reads, (20, 10, 5))
    assert 0 < int((out["kept"] == 0).sum()) < len(reads)


def test_reads_over_one_piece():
    """Five reads of 14 MiB: four fill a 64 MiB piece, the fifth goes up alone. A 10-letter bad tail, a 3-letter
    bad head and a dip of 7 letters below mask_q in each; the host model (C++) is the reference, the expectation is
    written down as well."""
    n, tail, head = 14 << 20, 10, 3
    q = np.full(n, 40 + 33, dtype=np.uint8)
    q[-tail:] = 2 + 33
    q[:head] = 2 + 33
    q[1000:1007] = 5 + 33
    qual = q.tobytes() * 5
    letters = (b"ACGT" * (n // 4)) * 5
    offs, lens = [k * n for k in range(5)], [n] * 5
    before = stage_qual_stats()
    got, out = quality_trim(letters, qual, offs, lens, 20, 10, 0)
    after = stage_qual_stats()
    host, host_out = quality_trim_host(letters, qual, offs, lens, 20, 10, 0)
    assert out.tolist() == host_out.tolist() == [(head, n - head - tail, 7, 0)] * 5
    assert got == host and got[1000:1007] == b"N" * 7 and got[4 * n + 1000:4 * n + 1007] == b"N" * 7
    assert after["launches"] - before["launches"] == 2 and after["masked"] - before["masked"] == 35
    assert after["trimmed3"] - before["trimmed3"] == 5 * tail and after["trimmed5"] - before["trimmed5"] == 5 * head


def test_off_parameters_and_no_reads_launch_nothing():
    reads = qc.random_set((20, 0, 0))[0][:40]
    check_stage(reads, (0, 0, 0))
    check_stage([], (20, 0, 0))
    before = stage_qual_stats()
    letters, qual, offs, lens = qc.lay_out(reads)
    got, out = quality_trim(letters, qual, offs, lens, 0, 0, 0)
    assert got == letters and out["kept"].tolist() == lens.tolist() and not out["bad"].any()
    assert stage_qual_stats() == before


REFUSALS = [
    ("param", dict(trim=94)), ("param", dict(mask=94)), ("param", dict(min_len=(1 << 24) + 1)),
    ("record", dict(offsets=[0, 99])), ("record", dict(lengths=[4, 95])), ("record", dict(offsets=[0, 1 << 40])),
    ("length", dict(big=True)),
]


@pytest.mark.parametrize("reason,change", REFUSALS)
def test_refusals_before_any_launch(reason, change):
    if change.get("big"):
        n = (1 << 24) + 1
        args = (b"A" * n, b"I" * n, [0], [n], 20, 0, 0)
    else:
        args = (b"ACGT" * 25, b"I" * 100, change.get("offsets", [0, 50]), change.get("lengths", [4, 50]),
                change.get("trim", 20), change.get("mask", 0), change.get("min_len", 0))
    before = stage_qual_stats()
    with pytest.raises(GhostmError, match="QualityTrimGpu: " + reason + ":"):
        quality_trim(*args)
    assert stage_qual_stats() == before
    with pytest.raises(GhostmError, match="GhostmQualityTrimHost: " + reason + ":"):
        quality_trim_host(*args)


# ------------------------------------------------------------------ session level
W, STEP = 127, 64


def all_records(s, width):
    out, c, total = [], 0, len(s.query_lengths())
    while sum(len(x) for x in out) < total:
        out.append(s.query_records(c).reshape(-1, width))
        c += 1
    return np.concatenate(out) if out else np.zeros((0, width), dtype=np.uint8)


@pytest.fixture(scope="module")
def plain_session():
    with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
        yield s


@pytest.mark.parametrize("params", [(20, 10, 30), (0, 15, 0), (2, 0, 0)])
def test_session_records(plain_session, params):
    s = plain_session
    reads = qc.random_set(params)[0]
    names = [f"r{k}" for k in range(len(reads))]
    seqs, quals = [x[0] for x in reads], [x[1] for x in reads]
    kw = dict(width=3 * W, dna=True, tile_step=STEP)
    want_out, trimmed = [], []
    for ls, qs in reads:
        new, rec, _ = qc.model_read(ls, qs, params)
        want_out.append(rec)
        trimmed.append(new[rec[0]:rec[0] + rec[1]])
    failed = [k for k, rec in enumerate(want_out) if rec[1] == 0 and len(reads[k][0]) > 0]
    assert len(failed) >= (20 if params[0] else 0) and any(rec[2] for rec in want_out) == bool(params[1])
    # the model's letters through the plain setter
    s.set_quality(0, 0, 0)
    s.set_queries(trimmed, names, **kw)
    want_records, want_tiles, want_lengths = all_records(s, W), s.query_tiles(), s.query_lengths()
    assert len(s.query_quality()) == 0 and s.quality_stats()["launches"] == 0
    # quality off: the quality-carrying set is the plain set of the untrimmed letters
    s.set_queries(seqs, names, quals=quals, **kw)
    off_records = all_records(s, W)
    assert len(s.query_quality()) == 0 and s.quality_stats()["launches"] == 0
    s.set_queries(seqs, names, **kw)
    assert all_records(s, W).tobytes() == off_records.tobytes() != want_records.tobytes()
    # quality on
    s.set_quality(*params)
    assert all_records(s, W).tobytes() == off_records.tobytes()  # the current set stays as it is
    s.set_queries(seqs, names, quals=quals, **kw)
    assert s.query_quality().tolist() == want_out
    assert all_records(s, W).tobytes() == want_records.tobytes()
    assert s.query_lengths().tolist() == want_lengths.tolist()
    # failed reads stay as records: the tile table, and with it every read's and mate's index, is the plain set's
    tiles = s.query_tiles()
    assert tiles.tobytes() == want_tiles.tobytes()
    assert sorted(set(int(t["record"]) for t in tiles)) == list(range(len(reads)))
    st = s.quality_stats()
    _, _, sums = qc.model(*qc.lay_out(reads), params)
    assert st["launches"] == 1 and st["seconds_quality"] > 0
    for k in COUNTERS[1:]:
        assert st[k] == sums[k], k
    # a refused setting leaves the old one in place; a plain set forgets the records
    for bad in ((94, 0, 0), (0, 94, 0), (0, 0, (1 << 24) + 1)):
        with pytest.raises(GhostmError, match="param:"):
            s.set_quality(*bad)
    s.set_queries(seqs, names, quals=quals, **kw)
    assert s.query_quality().tolist() == want_out
    s.set_queries(seqs, names, **kw)
    assert len(s.query_quality()) == 0 and s.quality_stats()["launches"] == 0
    s.set_quality(0, 0, 0)


def test_session_max_len_cuts_what_was_kept(plain_session):
    """Trimming comes first, then the cut: a read with a 5-letter bad head keeps letters 5..5 + 90."""
    s = plain_session
    ls = qc.rand_letters(random.Random(3), 200)
    qs = qc.to_qual([2] * 5 + [40] * 195)
    s.set_quality(20, 0, 0)
    s.set_queries([ls], ["a"], width=3 * W, dna=True, tile_step=STEP, max_len=90, quals=[qs])
    got = all_records(s, W)
    assert s.query_quality().tolist() == [(5, 195, 0, 0)]
    s.set_quality(0, 0, 0)
    s.set_queries([ls[5:95]], ["a"], width=3 * W, dna=True, tile_step=STEP)
    assert all_records(s, W).tobytes() == got.tobytes()


# ------------------------------------------------------------------ end to end
def back_translate(protein):
    first = {}
    for k, aa in enumerate(tc.CODONS):
        first.setdefault(aa, "".join("ACGT"[(k >> sh) & 3] for sh in (4, 2, 0)))
    return "".join(first[a] for a in protein)


def read_fasta(path):
    recs = []
    for block in open(path).read().split(">")[1:]:
        lines = block.split("\n")
        recs.append((lines[0].strip(), "".join(x.strip() for x in lines[1:])))
    return recs


def write_fastq(path, reads, newline="\n"):
    with open(path, "w", newline="") as f:
        for name, ls, qs in reads:
            f.write(f"@{name}{newline}{ls}{newline}+{newline}{qs}{newline}")


def write_fasta(path, recs):
    with open(path, "w") as f:
        for name, ls in recs:
            f.write(f">{name}\n{ls}\n")


PARAMS = (20, 0, 30)
KW = dict(width=3 * W, dna=True, tile_step=STEP)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("qual_e2e"))
    golden = dict(read_fasta(os.path.join(cases.GOLDEN, "testset_db.fasta")))      # the readme's DNA reads
    subjects = dict(read_fasta(os.path.join(cases.GOLDEN, "testset_queries.fasta")))  # and its database
    db = os.path.join(cases.GOLDEN, "testset_queries.fasta")
    tails = {"subject0": back_translate(subjects["query3"]), "subject2": back_translate(subjects["query4"])}
    reads = []  # (name, letters, quality text)
    for name in ("subject0", "subject3", "subject2", "subject4"):
        ls = golden[name]
        assert len(ls) == 75
        tail = tails.get(name, "")
        reads.append((name, ls + tail, "I" * len(ls) + "#" * len(tail)))
    reads.append(("junk", "ACGTTGCA" * 8, "#" * 64))    # all low: the ends cross
    reads.append(("short", "GCTGCTGCTGCTGCTGCTGCTGCT", "I" * 24))  # good, but under the floor
    trimmed = []
    for name, ls, qs in reads:
        new, rec, _ = qc.model_read(ls.encode(), qs.encode(), PARAMS)
        trimmed.append((name, new[rec[0]:rec[0] + rec[1]].decode()))
        # the model cuts exactly the appended part, empties junk and short, and leaves the rest alone
        want = (0, 0) if name in ("junk", "short") else (0, 75)
        assert rec[:2] == want and rec[2:] == (0, 0), (name, rec)
    res = dict(tmp=tmp, db=db, reads=reads, trimmed=trimmed)
    for key, recs in (("fa_full", [(n, ls) for n, ls, _ in reads]), ("fa_trimmed", trimmed)):
        res[key] = os.path.join(tmp, key + ".fa")
        write_fasta(res[key], recs)
    res["fq"] = os.path.join(tmp, "reads.fq")
    write_fastq(res["fq"], reads)
    res["fq_crlf"] = os.path.join(tmp, "reads_crlf.fq")
    write_fastq(res["fq_crlf"], reads, "\r\n")
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "12"]) as s:
        s.set_db_fasta(db)

        def run(setter):
            setter()
            s.run()
            return dict(text=s.output(), records=all_records(s, W), tiles=s.query_tiles(), quality=s.query_quality(),
                        stats=s.quality_stats())
        res["fasta_full"] = run(lambda: s.set_queries_fasta(res["fa_full"], **KW))
        res["fastq_off"] = run(lambda: s.set_queries_fastq(res["fq"], **KW))
        res["fasta_trimmed"] = run(lambda: s.set_queries_fasta(res["fa_trimmed"], **KW))
        s.set_quality(*PARAMS)
        res["fastq_on"] = run(lambda: s.set_queries_fastq(res["fq"], **KW))
        res["fastq_on_crlf"] = run(lambda: s.set_queries_fastq(res["fq_crlf"], **KW))
        # a refused file leaves the set as it was
        bad = os.path.join(tmp, "bad.fq")
        write_fastq(bad, [reads[0], ("x", "ACGT", "II\x7fI")])
        with pytest.raises(GhostmError, match=r"fastq: record 2: quality byte outside '!'\.\.'~'"):
            s.set_queries_fastq(bad, **KW)
        write_fastq(bad, [reads[0], ("x", "ACGT", "III")])
        with pytest.raises(GhostmError, match="fastq: record 2: 4 letters, 3 qualities"):
            s.set_queries_fastq(bad, **KW)
        with pytest.raises(GhostmError, match="fastq: record 1: header does not begin with '@'"):
            s.set_queries_fastq(res["fa_full"], **KW)
        res["after_refusals"] = dict(records=all_records(s, W), quality=s.query_quality())
    return res


def hits_of(text):
    out = {}
    for line in text.decode().splitlines():
        cols = line.split("\t")
        out.setdefault(cols[0], []).append(cols[1].strip())
    return out


def test_e2e_quality_off_is_the_fasta_set(e2e):
    a, b = e2e["fasta_full"], e2e["fastq_off"]
    assert len(a["text"]) > 0 and a["text"] == b["text"]
    assert a["records"].tobytes() == b["records"].tobytes() and a["tiles"].tobytes() == b["tiles"].tobytes()
    assert len(b["quality"]) == 0 and b["stats"]["launches"] == 0


def test_e2e_quality_on_is_the_fasta_of_the_trimmed_reads(e2e):
    a, b = e2e["fasta_trimmed"], e2e["fastq_on"]
    assert len(a["text"]) > 0 and a["text"] == b["text"]
    assert a["records"].tobytes() == b["records"].tobytes() and a["tiles"].tobytes() == b["tiles"].tobytes()
    assert b["quality"].tolist() == [(0, 75, 0, 0), (0, 75, 0, 0), (0, 75, 0, 0), (0, 75, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    st = b["stats"]
    assert (st["launches"], st["reads"], st["failed"], st["trimmed5"], st["masked"]) == (1, 6, 2, 0, 0)
    assert st["trimmed3"] == 75 + 75 + 64 + 24 and st["letters"] == 4 * 75 + 150 + 64 + 24
    c = e2e["fastq_on_crlf"]
    assert c["text"] == b["text"] and c["quality"].tolist() == b["quality"].tolist()
    r = e2e["after_refusals"]
    assert r["records"].tobytes() == c["records"].tobytes() and r["quality"].tolist() == c["quality"].tolist()


def test_e2e_a_low_quality_tail_no_longer_hits(e2e):
    off, on = hits_of(e2e["fastq_off"]["text"]), hits_of(e2e["fastq_on"]["text"])
    assert "query3" in off["subject0"] and "query3" not in on["subject0"]   # the tail's subject
    assert "query4" in off["subject2"] and "query4" not in on["subject2"]
    # trimmed, the two reads hit what the golden answer (readme_kat.out) lists for them
    assert on["subject0"] == ["query0", "query6"] and on["subject2"] == ["query5", "query6"]
    assert off["subject0"] != on["subject0"] and off["subject2"] != on["subject2"]
    assert on["subject3"] == off["subject3"] and "junk" not in on and "short" not in on


def test_e2e_cli(e2e):
    base = [native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-y", "12", "-q", "d", "-w", str(3 * W), "-T", str(STEP)]
    tmp = e2e["tmp"]
    for on in (False, True):
        out = os.path.join(tmp, f"cli_{int(on)}.out")
        p = subprocess.run(base + (["-Q", "20,0,30", "-v"] if on else []) + [e2e["fq"], out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert open(out, "rb").read() == e2e["fastq_on" if on else "fastq_off"]["text"]
        if on:
            st = e2e["fastq_on"]["stats"]
            assert f"quality trimmed 5' 0 3' {st['trimmed3']} masked 0 failed reads 2 of 6 seconds" in p.stdout
    out = os.path.join(tmp, "bad.out")
    for bad in ("1,2", "99,0,0", "20,94,0", "20,0,16777217", "20,,0", "a,0,0", "20,0,0,1", ""):
        p = subprocess.run(base + ["-Q", bad, e2e["fq"], out], capture_output=True, text=True)
        assert p.returncode == 1, bad
    # a FASTQ file without -T: the sample's message, and the command goes on
    p = subprocess.run([native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-q", "d", "-w", str(3 * W), e2e["fq"], out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and "fastq: needs -T" in p.stderr and open(out, "rb").read() == b""
    # -Q on a FASTA file
    p = subprocess.run(base + ["-Q", "20,0,30", e2e["fa_full"], out], capture_output=True, text=True)
    assert p.returncode == 0 and f"quality: {e2e['fa_full']} has no qualities" in p.stderr
    # aln does not take it
    p = subprocess.run([native.BIN_PATH, "aln", "-Q", "20,0,30", "-i", "x", "-d", "y", "-o", os.devnull],
                       capture_output=True, text=True)
    assert "quality" not in p.stdout


def test_e2e_cli_mates_in_two_fastq_files(e2e):
    """-J r1.fastq r2.fastq prints what -j prints for the interleaved FASTA of the trimmed mates; the emptied mates
    (junk in r1, short in r2) stay records, so every pair keeps its partner."""
    tmp, reads, trimmed = e2e["tmp"], e2e["reads"], dict(e2e["trimmed"])
    order1, order2 = ["subject0", "subject3", "junk"], ["subject4", "subject2", "short"]
    by_name = {r[0]: r for r in reads}
    r1, r2, fa = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq"), os.path.join(tmp, "mates.fa")
    write_fastq(r1, [by_name[n] for n in order1])
    write_fastq(r2, [by_name[n] for n in order2])
    write_fasta(fa, [(n, trimmed[n]) for pair in zip(order1, order2) for n in pair])
    base = [native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-y", "12", "-q", "d", "-w", str(3 * W), "-T", str(STEP)]
    out_j, out_J = os.path.join(tmp, "j.out"), os.path.join(tmp, "J.out")
    p = subprocess.run(base + ["-j", fa, out_j], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    p = subprocess.run(base + ["-J", "-Q", "20,0,30", r1, r2, out_J], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    text = open(out_J, "rb").read()
    assert len(text) > 0 and text == open(out_j, "rb").read()
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "12"]) as s:
        s.set_db_fasta(e2e["db"])
        s.set_mates(True, 1000)
        s.set_quality(*PARAMS)
        s.set_queries_fastq_mates(r1, r2, **KW)
        assert s.query_quality()["kept"].tolist() == [75, 75, 75, 75, 0, 0]
        assert sorted(set(int(t["record"]) for t in s.query_tiles())) == list(range(6))
        s.run()
        assert s.output() == text
        with pytest.raises(GhostmError, match=r"mates: .* has 3 records, .* has 6"):
            s.set_queries_fastq_mates(r1, e2e["fq"], **KW)
        assert s.query_quality()["kept"].tolist() == [75, 75, 75, 75, 0, 0]
