"""Adapter removal for FASTQ reads on the GPU (k_adapter_find, k_pair_overlap,
ghostm_amd/csrc/read_adapter.hip; AdapterTrimGpu, GhostmSessionSetAdapters,
GhostmSessionSetQueriesFastq*Tiled, `ghostm search -A -O`).

Stage level: adapter_trim against adapter_trim_host and the Python model of
adapter_cases.py, every field of every record, on every case set and named
case; the counters move by the model's sums; the letters stay as they were;
launches with more reads and more pairs than waves; reads over one upload piece
with the pair rule on; every refusal before any launch. Session level:
set_adapters with set_queries(..., quals=...) and with set_queries_fastq_mates
gives the model's records, the query records of the reads cut by hand, and with
quality on the quality model's records of the cut reads. End to end on the
golden testset (the readme's database, testset_queries.fasta, and its DNA
reads, testset_db.fasta): a FASTQ of the golden reads, some cut to a fragment
and read through into the adapter, alone and as R1/R2 files.

The kernels use no LDS (the file's header comment says so), so there is no run
under the LDS-poison build."""
import os
import random
import subprocess

import numpy as np
import pytest

import adapter_cases as ac
import cases
import qual_cases as qc
from ghostm_amd import GhostmError, adapter_trim, adapter_trim_host, native, stage_adapter_stats
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

COUNTERS = ("launches",) + ac.SUM_KEYS


def kernels_of(params):
    a1, a2, _, _, po = params
    return int(bool(a1 or a2)) + int(bool(po))


def check_stage(reads, params, filler=b"#"):
    letters, offs, lens = ac.lay_out(reads, filler)
    buf = bytearray(letters)
    before = stage_adapter_stats()
    out = adapter_trim(buf, offs, lens, *params)
    after = stage_adapter_stats()
    host = adapter_trim_host(letters, offs, lens, *params)
    assert out.tolist() == host.tolist()
    assert bytes(buf) == letters  # the letters stay untouched
    want, sums = ac.model_reads(reads, params)
    assert out.tolist() == want.tolist()
    delta = {k: after[k] - before[k] for k in COUNTERS}
    on = kernels_of(params) > 0 and len(reads) > 0
    assert delta["launches"] == (kernels_of(params) if on else 0)  # one piece
    for k in ac.SUM_KEYS:
        assert delta[k] == (sums[k] if on else 0), k
    assert after["seconds_adapter"] > before["seconds_adapter"] or not on
    return out


# ------------------------------------------------------------------ stage level
@pytest.mark.parametrize("m,mo,err", ac.ADAPTER_SETS)
def test_adapter_sets_equal_host_and_model(m, mo, err):
    reads, adapter = ac.fixed_set(m, mo)
    check_stage(reads, ac.P(adapter, b"", mo, err), adapter)
    reads, adapter = ac.random_set(m, mo, err)
    check_stage(reads, ac.P(adapter, b"", mo, err), adapter)
    check_stage(reads, ac.P(ac.adapter_of(33, 1), adapter, mo, err), adapter)


@pytest.mark.parametrize("po,err", ac.PAIR_SETS)
def test_pair_sets_equal_host_and_model(po, err):
    reads = ac.random_pairs(po, err)
    check_stage(reads, ac.P(b"", b"", 5, err, po), ac.TRUSEQ)
    check_stage(reads, ac.P(ac.TRUSEQ, ac.TRUSEQ2, 5, err, po), ac.TRUSEQ)


@pytest.mark.parametrize("name", sorted(ac.named_cases()))
def test_named_cases(name):
    reads, params, want = ac.named_cases()[name]
    out = check_stage(reads, params, params[0] or b"#")
    if want is not None:
        assert [(int(o["kept"]), int(o["adapter_at"]), int(o["pair_len"])) for o in out] == want


def test_more_reads_than_waves():
    reads = ac.grid_stride_set()
    assert len(reads) > 4 * 1024  # kAdapterBlocksMax blocks of four waves
    out = check_stage(reads, ac.P(ac.TRUSEQ, b"", 5, 10, 0), ac.TRUSEQ)
    assert 500 < int((out["kept"] < [len(r) for r in reads]).sum()) < len(reads)


def test_more_pairs_than_waves():
    reads = ac.grid_stride_pairs()
    assert len(reads) // 2 > 4 * 1024
    out = check_stage(reads, ac.P(ac.TRUSEQ, ac.TRUSEQ2, 5, 10, 8), ac.TRUSEQ)
    assert 500 < int((out["pair_len"][0::2] > 0).sum()) < len(reads) // 2


def test_reads_over_one_piece_with_the_pair_rule_on():
    """Six reads of 12 MiB, the pair rule on: a piece holds whole pairs, so two pairs (48 MiB) fill the first
    64 MiB piece and the third goes up alone, where five single reads would have fitted; two kernels per piece.
    Every mate is over 1024 letters, so the three pairs are skipped and counted. The adapter lies 2000 letters
    into reads 0..4 and 40 letters before the end of read 5, which is walked whole. The host model (C++) is the
    reference, the expectation is written down as well."""
    n = 12 << 20
    adapter = b"AGATCGGAAGAGC"  # in no stretch of ACGTACGT...
    base = b"ACGT" * (n // 4)
    near, far = 2000, n - 40
    first = base[:near] + adapter + base[near + len(adapter):]
    last = base[:far] + adapter + base[far + len(adapter):]
    letters = first * 5 + last
    offs, lens = [k * n for k in range(6)], [n] * 6
    params = ac.P(adapter, b"", 5, 10, 20)
    before = stage_adapter_stats()
    out = adapter_trim(letters, offs, lens, *params)
    after = stage_adapter_stats()
    host = adapter_trim_host(letters, offs, lens, *params)
    assert out.tolist() == host.tolist() == [(near, near, 0, 0, 0)] * 5 + [(far, far, 0, 0, 0)]
    delta = {k: after[k] - before[k] for k in COUNTERS}
    assert delta["launches"] == 2 * 2 and delta["pair_skipped"] == 3 and delta["pair_found"] == 0
    assert delta["reads"] == 6 and delta["letters"] == 6 * n and delta["adapter_found"] == delta["cut_reads"] == 6
    assert delta["cut_letters"] == 5 * (n - near) + 40 and delta["emptied"] == 0


def test_off_parameters_and_no_reads_launch_nothing():
    reads = ac.random_set(33, 5, 10)[0][:40]
    before = stage_adapter_stats()
    check_stage(reads, ac.P())
    check_stage([], ac.P(ac.TRUSEQ))
    check_stage([], ac.P(ac.TRUSEQ, b"", 5, 10, 20))
    letters, offs, lens = ac.lay_out(reads)
    out = adapter_trim(letters, offs, lens)
    assert out["kept"].tolist() == out["adapter_at"].tolist() == lens.tolist() and not out["pair_len"].any()
    assert stage_adapter_stats() == before


@pytest.mark.parametrize("reason,change", ac.REFUSALS)
def test_refusals_before_any_launch(reason, change):
    args = ac.refusal_args(change)
    before = stage_adapter_stats()
    with pytest.raises(GhostmError, match="AdapterTrimGpu: " + reason + ":"):
        adapter_trim(*args)
    assert stage_adapter_stats() == before
    with pytest.raises(GhostmError, match="GhostmAdapterTrimHost: " + reason + ":"):
        adapter_trim_host(*args)


# ------------------------------------------------------------------ session level
W, STEP = 127, 64
KW = dict(width=3 * W, dna=True, tile_step=STEP)


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


def session_reads():
    """Pairs with read-through and their adapters behind the fragment, upper case, and a quality string each with a
    low tail on some."""
    rnd = random.Random(41)
    reads = []
    for k in range(60):
        n1, n2 = rnd.randint(60, 260), rnd.randint(60, 260)
        if k % 3 == 0:
            reads += [ac.rand_letters(rnd, n1), ac.rand_letters(rnd, n2)]
        else:
            reads += list(ac.read_through(rnd, rnd.randint(25, min(n1, n2)), n1, n2, errors=k % 2))
    quals = [qc.to_qual(qc.profile(rnd, len(r), ("untouched", "tail", "both")[k % 3], 20)) for k, r in enumerate(reads)]
    return reads, quals


SESSION_PARAMS = [ac.P(ac.TRUSEQ, ac.TRUSEQ2, 5, 10, 20), ac.P(ac.TRUSEQ, b"", 5, 10, 0), ac.P(b"", b"", 5, 10, 20)]


@pytest.mark.parametrize("params", SESSION_PARAMS)
@pytest.mark.parametrize("quality", [(0, 0, 0), (20, 10, 30)])
def test_session_records(plain_session, params, quality):
    s = plain_session
    reads, quals = session_reads()
    names = [f"r{k}" for k in range(len(reads))]
    want, sums = ac.model_reads(reads, params)
    kept = [int(k) for k in want["kept"]]
    assert sum(k < len(r) for k, r in zip(kept, reads)) >= 30 and sum(k == len(r) for k, r in zip(kept, reads)) >= 30
    cut = [r[:k] for r, k in zip(reads, kept)]
    cut_quals = [q[:k] for q, k in zip(quals, kept)]
    # the reads cut by hand, adapters off
    s.set_adapters()
    s.set_quality(*quality)
    s.set_queries(cut, names, quals=cut_quals, **KW)
    want_records, want_tiles, want_quality = all_records(s, W), s.query_tiles(), s.query_quality()
    assert len(s.query_adapters()) == 0 and s.adapter_stats()["launches"] == 0
    s.set_queries(reads, names, quals=quals, **KW)
    off_records = all_records(s, W)
    assert off_records.tobytes() != want_records.tobytes() and len(s.query_adapters()) == 0
    # adapters on
    s.set_adapters(*params)
    assert all_records(s, W).tobytes() == off_records.tobytes()  # the current set stays as it is
    s.set_queries(reads, names, quals=quals, **KW)
    assert s.query_adapters().tolist() == want.tolist()
    assert all_records(s, W).tobytes() == want_records.tobytes()
    assert s.query_tiles().tobytes() == want_tiles.tobytes()
    assert sorted(set(int(t["record"]) for t in s.query_tiles())) == list(range(len(reads)))
    # the quality stage saw the cut reads: the quality model on them
    got_quality = s.query_quality()
    assert got_quality.tolist() == want_quality.tolist()
    if any(quality):
        model_q = [qc.model_read(c, q, quality)[1] for c, q in zip(cut, cut_quals)]
        assert got_quality.tolist() == model_q and any(rec[0] or rec[1] < len(c) for rec, c in zip(model_q, cut))
    else:
        assert len(got_quality) == 0
    st = s.adapter_stats()
    assert st["launches"] == kernels_of(params) and st["seconds_adapter"] > 0
    for k in ac.SUM_KEYS:
        assert st[k] == sums[k], k
    # a refused setting leaves the old one in place
    for bad in (dict(min_overlap=0), dict(err_pct=51), dict(pair_overlap=1025), dict(adapter1="ACGU"), dict(adapter2="A" * 65)):
        with pytest.raises(GhostmError, match="adapters: (param|adapter):"):
            s.set_adapters(**bad)
    s.set_queries(reads, names, quals=quals, **KW)
    assert s.query_adapters().tolist() == want.tolist()
    # a protein set and, with the pair rule on, an odd set are refused, and the set stays
    with pytest.raises(GhostmError, match="adapters: a protein set"):
        s.set_queries([b"MKV" * 30], ["p"], quals=[b"I" * 90], width=W, dna=False, tile_step=STEP)
    if params[4]:
        with pytest.raises(GhostmError, match="adapters: pairs:"):
            s.set_queries(reads[:3], names[:3], quals=quals[:3], **KW)
    assert s.query_adapters().tolist() == want.tolist() and all_records(s, W).tobytes() == want_records.tobytes()
    # a plain set forgets the records
    s.set_queries(reads, names, **KW)
    assert len(s.query_adapters()) == 0 and s.adapter_stats()["launches"] == 0
    s.set_adapters()
    s.set_quality(0, 0, 0)


# ------------------------------------------------------------------ end to end
def read_fasta(path):
    recs = []
    for block in open(path).read().split(">")[1:]:
        lines = block.split("\n")
        recs.append((lines[0].strip(), "".join(x.strip() for x in lines[1:])))
    return recs


def write_fastq(path, reads):
    with open(path, "w") as f:
        for name, ls in reads:
            f.write(f"@{name}\n{ls}\n+\n{'I' * len(ls)}\n")


def write_fasta(path, recs):
    with open(path, "w") as f:
        for name, ls in recs:
            f.write(f">{name}\n{ls}\n")


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("adapter_e2e"))
    db = os.path.join(cases.GOLDEN, "testset_queries.fasta")  # the readme's database
    single, pairs = ac.e2e_reads(dict(read_fasta(os.path.join(cases.GOLDEN, "testset_db.fasta"))))
    (single_out, single_sums), (pairs_out, pairs_sums) = ac.check_e2e(single, pairs)
    res = dict(tmp=tmp, db=db, single=single, pairs=pairs, single_out=single_out, pairs_out=pairs_out,
               single_sums=single_sums, pairs_sums=pairs_sums)
    text = lambda reads, cut: [(n, (ls[:k] if cut else ls).decode()) for n, ls, k in reads]  # noqa: E731
    for key, reads in (("single", single), ("r1", pairs[0::2]), ("r2", pairs[1::2])):
        for cut in (False, True):
            path = os.path.join(tmp, f"{key}_{'cut' if cut else 'full'}.fq")
            write_fastq(path, text(reads, cut))
            res[f"{key}_{'cut' if cut else 'full'}"] = path
    res["single_fa"] = os.path.join(tmp, "single_full.fa")
    write_fasta(res["single_fa"], text(single, False))
    # a taxonomy over the database: every subject a species of one genus
    subjects = [n for n, _ in read_fasta(db)]
    res["nodes"], res["map"] = os.path.join(tmp, "nodes.tsv"), os.path.join(tmp, "map.tsv")
    with open(res["nodes"], "w") as f:
        f.write("1\t1\n10\t1\n" + "".join(f"{100 + k}\t10\n" for k in range(len(subjects))))
    with open(res["map"], "w") as f:
        f.write("".join(f"{n}\t{100 + k}\n" for k, n in enumerate(subjects)))
    return res


def search(e2e, y, extra, files, out_name):
    out = os.path.join(e2e["tmp"], out_name)
    cmd = [native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-q", "d", "-w", str(3 * W), "-T", str(STEP), "-y", str(y),
           "-n", e2e["nodes"], "-a", e2e["map"]] + extra + files + [out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    return p, (open(out, "rb").read() if os.path.exists(out) else None)


A_SINGLE = ["-A", ac.TRUSEQ.decode(), "-O", "5,10"]
A_PAIRS = ["-A", ac.TRUSEQ.decode() + "," + ac.TRUSEQ2.decode(), "-O", "5,10,20"]


@pytest.mark.parametrize("y", [13, 23])
def test_e2e_cli_single_file_equals_the_reads_cut_by_hand(e2e, y):
    """`search -A ... -O ...` on the reads with adapter tails writes the bytes of the same command without them on
    the reads cut by hand. The untrimmed run prints another text on this testset, for both styles."""
    p, got = search(e2e, y, A_SINGLE + ["-v"], [e2e["single_full"]], f"s{y}_on.out")
    assert p.returncode == 0 and "adapters" not in p.stderr, p.stderr
    q, want = search(e2e, y, [], [e2e["single_cut"]], f"s{y}_cut.out")
    assert q.returncode == 0 and q.stderr == p.stderr, q.stderr
    assert got is not None and len(got) > 0 and got == want
    _, untrimmed = search(e2e, y, [], [e2e["single_full"]], f"s{y}_off.out")
    assert untrimmed is not None and untrimmed != got
    sums = e2e["single_sums"]
    assert (f"# {e2e['single_full']} adapters cut reads {sums['cut_reads']} letters {sums['cut_letters']} adapter found "
            f"{sums['adapter_found']} pairs found 0 skipped 0 emptied {sums['emptied']} of {sums['reads']} seconds") in p.stdout
    assert "adapters" not in q.stdout


def test_e2e_cli_two_files_of_mates(e2e):
    """-J with both adapters and the pair rule, -y 27 (and -y 13 for the read-level lines): the bytes of the run on
    the mates cut by hand. The untrimmed run prints another text on this testset, for both styles."""
    for y in (27, 13):
        p, got = search(e2e, y, ["-J"] + A_PAIRS + ["-v"], [e2e["r1_full"], e2e["r2_full"]], f"J{y}_on.out")
        assert p.returncode == 0 and "adapters" not in p.stderr, p.stderr
        q, want = search(e2e, y, ["-J"], [e2e["r1_cut"], e2e["r2_cut"]], f"J{y}_cut.out")
        assert q.returncode == 0 and q.stderr == p.stderr, q.stderr
        assert got is not None and len(got) > 0 and got == want
        _, untrimmed = search(e2e, y, ["-J"], [e2e["r1_full"], e2e["r2_full"]], f"J{y}_off.out")
        assert untrimmed is not None and untrimmed != got
        sums = e2e["pairs_sums"]
        assert (f"adapters cut reads {sums['cut_reads']} letters {sums['cut_letters']} adapter found "
                f"{sums['adapter_found']} pairs found {sums['pair_found']} skipped 0 emptied 0 of 10 seconds") in p.stdout
        if y == 27:  # the pair rule alone finds the same cuts here
            p, alone = search(e2e, y, ["-J", "-O", "5,10,20"], [e2e["r1_full"], e2e["r2_full"]], "J27_pair_only.out")
            assert p.returncode == 0 and alone == want


def test_e2e_session_mates_and_the_default_path(e2e):
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "13"]) as s:
        s.set_db_fasta(e2e["db"])
        # the stage never set: nothing is launched, and a FASTQ file gives the FASTA file's set and text
        s.set_queries_fastq(e2e["single_full"], **KW)
        s.run()
        text, records = s.output(), all_records(s, W)
        assert s.adapter_stats()["launches"] == 0 and len(s.query_adapters()) == 0 and len(text) > 0
        s.set_queries_fasta(e2e["single_fa"], **KW)
        s.run()
        assert s.output() == text and all_records(s, W).tobytes() == records.tobytes()
        # two files of mates: the pairing is that of the interleaved records
        s.set_adapters(*ac.E2E_PAIRS)
        s.set_queries_fastq_mates(e2e["r1_full"], e2e["r2_full"], **KW)
        assert s.query_adapters().tolist() == e2e["pairs_out"].tolist()
        on = all_records(s, W)
        st = s.adapter_stats()
        assert st["launches"] == 2 and all(st[k] == e2e["pairs_sums"][k] for k in ac.SUM_KEYS)
        s.set_adapters()
        s.set_queries_fastq_mates(e2e["r1_cut"], e2e["r2_cut"], **KW)
        assert all_records(s, W).tobytes() == on.tobytes() and s.adapter_stats()["launches"] == 0


def test_e2e_cli_usage_errors_and_refusals(e2e):
    out = os.path.join(e2e["tmp"], "bad.out")
    base = [native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-q", "d", "-w", str(3 * W), "-T", str(STEP)]
    ad = ac.TRUSEQ.decode()
    for bad in (["-A", ""], ["-A", "ACGU"], ["-A", "A" * 65], ["-A", ad + ","], ["-A", "," + ad], ["-A", ad + "," + ad],
                ["-A", ad, "-O", "5"], ["-A", ad, "-O", "0,10"], ["-A", ad, "-O", "65,10"], ["-A", ad, "-O", "5,51"],
                ["-A", ad, "-O", "5,10,"], ["-A", ad, "-O", "5,,10"], ["-A", ad, "-O", "a,10"], ["-A", ad, "-O", "5,10,20,1"],
                ["-A", ad, "-O", "5,10,20"], ["-j", "-A", ad, "-O", "5,10,1025"], ["-O", "5,10"], ["-O", "5,10,0"],
                ["-O", "5,10,20"]):
        p = subprocess.run(base + bad + [e2e["single_full"], out], capture_output=True, text=True)
        assert p.returncode == 1, bad
    # a FASTA sample with the stage on: the sample's message, and the command goes on
    p = subprocess.run(base + ["-A", ad, e2e["single_fa"], out], capture_output=True, text=True)
    assert p.returncode == 0 and f"adapters: {e2e['single_fa']} is not FASTQ" in p.stderr
    # the pair rule on an odd file
    p = subprocess.run(base + ["-j", "-O", "5,10,20", e2e["single_full"], out], capture_output=True, text=True)
    assert p.returncode == 0 and "adapters: pairs: 7 records" in p.stderr
