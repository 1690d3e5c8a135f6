"""Low-complexity masking on the GPU (k_mask_windows + k_mask_apply,
ghostm_amd/csrc/query_mask.hip; MaskRecordsGpu, GhostmSessionSetMask, `ghostm
search -Z`).

Stage level: mask_records against mask_records_host (and the Python model of
mask_cases.py) byte for byte on every case set and on the carry cases by name;
every refusal before any launch. Session level: set_mask then set_queries gives
the model applied to the unmasked set's records, lengths unchanged, and nothing
runs while masking is off. End to end: a read whose only similarity to a subject
is a low-complexity stretch loses its hit, a read with a real domain keeps it,
and the CLI prints the session's lines. The kernels under LDS poison."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import cases
import mask_cases as mc
from ghostm_amd import GhostmError, mask_records, mask_records_host, native, stage_mask_stats
from ghostm_amd.aligner import Session

pytestmark = pytest.mark.gpu

COUNTERS = ("mask_launches", "mask_sources", "mask_windows", "masked_sources", "masked_letters")


def check_stage(records, srcs, W, step, w, levels, want=None, counts=None, per_source=None):
    before = stage_mask_stats()
    got, masked = mask_records(records, W, srcs, step, w, *levels)
    after = stage_mask_stats()
    host, host_masked = mask_records_host(records, W, srcs, step, w, *levels)
    assert got.tobytes() == host.tobytes() and masked.tobytes() == host_masked.tobytes()
    if want is not None:
        assert got.tobytes() == want.tobytes() and masked.tolist() == counts.tolist()
    with_windows = [int(s["letters"]) - w + 1 for s in srcs if int(s["letters"]) >= w]
    delta = {k: after[k] - before[k] for k in COUNTERS}
    assert delta["mask_launches"] == (1 if with_windows else 0)
    assert delta["mask_sources"] == len(with_windows) and delta["mask_windows"] == sum(with_windows)
    if per_source is not None:
        assert delta["masked_sources"] == sum(1 for n in per_source if n) and delta["masked_letters"] == sum(per_source)
    assert after["seconds_mask"] > before["seconds_mask"] or not with_windows


# ------------------------------------------------------------------ stage level
@pytest.mark.parametrize("w,levels,layout", mc.all_case_sets())
def test_stage_equals_host_model(w, levels, layout):
    records, srcs, step, want, counts, per_source = mc.case_set(w, levels, layout)
    check_stage(records, srcs, layout[0], step, w, levels, want, counts, per_source)


@pytest.mark.parametrize("name", sorted(mc.carry_cases()))
def test_carry_cases(name):
    letters, W, step, stride, w, levels, check = mc.carry_cases()[name]
    low, trig = mc.flags(letters[0], w, *levels)
    check(low, trig, mc.mask_letters(letters[0], w, *levels))
    records, srcs = mc.lay_out(letters, W, step, stride)
    want, counts, per_source = mc.model(records, srcs, W, step, w, *levels)
    check_stage(records, srcs, W, step, w, levels, want, counts, per_source)


def test_dna_frames_with_a_stop_run():
    frames = mc.dna_carry_case()
    for W, step in ((40, 7), (127, 64)):
        records, srcs = mc.lay_out(frames, W, step, 6)
        want, counts, per_source = mc.model(records, srcs, W, step, 12, 220, 250)
        assert sum(1 for n in per_source if n) >= 3 and (records == mc.STAR).any()
        check_stage(records, srcs, W, step, 12, (220, 250), want, counts, per_source)


def test_no_source_with_a_window_launches_nothing():
    records, srcs = mc.lay_out([[3] * 11] * 6, 20, 7, 6)
    check_stage(records, srcs, 20, 7, 12, (0, 500))
    got, masked = mask_records(records, 20, srcs[:0], 7, 12, 220, 250)
    assert got.tobytes() == records.tobytes() and not masked.any()


@pytest.mark.parametrize("reason,change", mc.REFUSALS + [("source", dict(width=128))])
def test_refusals_before_any_launch(reason, change):
    records, src, args = mc.refusal_args(change)
    W = args.get("width", 20)
    if W != 20:
        records, src = np.full((1, W), 5, dtype=np.uint8), np.array([(0, 1, 1, W)], dtype=mc.SOURCE_DTYPE)
    before = stage_mask_stats()
    with pytest.raises(GhostmError, match=reason + ":"):
        mask_records(records, W, src, args["step"], args["window"], args["trigger"], args["extend"])
    assert stage_mask_stats() == before
    if W == 20:  # the host model names the same reason
        with pytest.raises(GhostmError, match=reason + ":"):
            mask_records_host(records, W, src, args["step"], args["window"], args["trigger"], args["extend"])


# ------------------------------------------------------------------ session level
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


@pytest.mark.parametrize("name", ["protein_untiled", "protein_tiled", "dna_tiled"])
@pytest.mark.parametrize("params", [(12, 220, 250), (6, 0, 500)])
def test_session_records(plain_session, name, params):
    s = plain_session
    seqs, names, kw, W, step = mc.session_sets()[name]
    s.set_mask(0)
    s.set_queries(seqs, names, **kw)
    plain, lengths = all_records(s, W), s.query_lengths()
    assert len(s.query_masked()) == 0 and s.mask_stats()["mask_launches"] == 0
    srcs = mc.session_sources(s.query_tiles(), len(plain), W, kw.get("dna", False))
    want, counts, per_source = mc.model(plain, srcs, W, step or W, *params)
    assert 0 < sum(1 for n in per_source if n) < len(per_source)
    s.set_mask(*params)
    assert all_records(s, W).tobytes() == plain.tobytes()  # the current set stays as it is
    s.set_queries(seqs, names, **kw)
    got = all_records(s, W)
    assert got.tobytes() == want.tobytes()
    assert s.query_lengths().tolist() == lengths.tolist()
    assert s.query_masked().tolist() == counts.tolist()
    st = s.mask_stats()
    assert st["mask_launches"] == 1 and st["seconds_mask"] > 0
    assert st["mask_sources"] == sum(1 for x in srcs if int(x["letters"]) >= params[0])
    assert st["masked_sources"] == sum(1 for n in per_source if n) and st["masked_letters"] == sum(per_source)
    # a refused setting leaves the old one in place
    for bad, reason in (((5, 220, 250), "window"), ((12, 300, 200), "levels"), ((12, 0, 501), "levels")):
        with pytest.raises(GhostmError, match=reason + ":"):
            s.set_mask(*bad)
    s.set_queries(seqs, names, **kw)
    assert all_records(s, W).tobytes() == want.tobytes()
    s.set_mask(0)
    s.set_queries(seqs, names, **kw)
    assert all_records(s, W).tobytes() == plain.tobytes()
    assert len(s.query_masked()) == 0 and s.mask_stats()["mask_launches"] == 0


def test_masking_never_set_changes_nothing(dataset):
    """-y 0 against the CPU oracle as ever, and -y 22 equal to a session that set masking and turned it off again;
    no mask launch in either."""
    d = dataset("protein_testset")
    out = {}
    for y in ("0", "22"):
        for touched in (False, True):
            with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0", "-y", y]) as s:
                if touched:
                    s.set_mask(12, 220, 250)
                    s.set_mask(0)
                if y == "22":
                    nsubj = sum(c["nseq"] for c in s.db_chunks())
                    s.set_taxonomy([1, 2, 3], [0, 0, 0], [1 + k % 2 for k in range(nsubj)])
                s.set_queries_fasta(os.path.join(cases.GOLDEN, "testset_queries.fasta"), width=75)
                s.run()
                out[y, touched] = s.output()
                assert s.mask_stats()["mask_launches"] == 0 and len(s.query_masked()) == 0
                assert len(out[y, touched]) > 0
        assert out[y, False] == out[y, True]
    with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
        s.run()
        assert s.output() == out["0", False]  # the set made from FASTA prints what the formatted files print
        assert s.mask_stats()["mask_launches"] == 0
    ref = os.path.join(d, "mask_oracle.out")
    subprocess.run([cases.ORACLE, "aln", "-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", ref], check=True)
    assert open(ref, "rb").read() == out["0", False]


# ------------------------------------------------------------------ end to end
AA = "ARNDCQEGHILKMFPSTWYV"


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    r = random.Random(4242)
    rand = lambda n: "".join(r.choice(AA) for _ in range(n))  # noqa: E731
    L = "".join(r.choice("QASP") for _ in range(40))
    D = rand(90)
    subjects = [("S1", rand(30) + L + rand(30)), ("S2", D)]
    Dm = list(D)
    for p in (11, 37, 70):
        Dm[p] = "W" if Dm[p] != "W" else "F"
    reads = [("A", rand(25) + L + rand(25)), ("B", "".join(Dm) + L)]
    tmp = tmp_path_factory.mktemp("mask_e2e")
    db, q = os.path.join(str(tmp), "db.fa"), os.path.join(str(tmp), "q.fa")
    for path, recs in ((db, subjects), (q, reads)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(f">{name}\n{seq}\n")
    res = dict(L=L, D=D, db=db, q=q, tmp=str(tmp), reads=reads)
    with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "14"]) as s:
        s.set_db([x[1] for x in subjects], [x[0] for x in subjects])
        for on in (False, True):
            s.set_mask(12, 220, 250) if on else s.set_mask(0)
            s.set_queries([x[1] for x in reads], [x[0] for x in reads], width=64, tile_step=32)
            s.run()
            res[on] = dict(text=s.output(), records=all_records(s, 64), tiles=s.query_tiles(), stats=s.mask_stats())
    return res


def lines_of(text):
    return [x.split("\t") for x in text.decode().splitlines()]


def test_e2e_low_complexity_hit_goes_real_hit_stays(e2e):
    off = lines_of(e2e[False]["text"])
    assert any(x[0] == "A" and x[1] == "S1" for x in off)  # masking off: A hits S1 through L alone
    on = lines_of(e2e[True]["text"])
    assert not any(x[0] == "A" for x in on)                 # masking on: A has no hit at all
    b = [x for x in on if x[0] == "B"]
    assert len(b) == 1 and b[0][1] == "S2"                  # and B still hits S2
    # B's read as masked: X over L in every tile that covers it
    L0 = len(e2e["D"])
    masked_read = {}
    for i, t in enumerate(e2e[True]["tiles"]):
        if int(t["record"]) == 1:
            for k in range(min(64, int(t["letters"]) - int(t["offset"]))):
                letter = mc.ORDER[int(e2e[True]["records"][i, k])]
                assert masked_read.setdefault(int(t["offset"]) + k, letter) == letter
    assert all(masked_read[p] == "X" for p in range(L0, L0 + 40))
    assert sum(1 for p in range(L0) if masked_read[p] == "X") < 12
    # the -y 14 line: q_end lies before L, and qseq is the masked read over the aligned stretch
    qstart, qend, qseq = int(b[0][6]), int(b[0][7]), b[0][14]
    assert qend <= L0
    letters = [c for c in qseq if c != "-"]
    assert letters == [masked_read[p] for p in range(qstart - 1, qend)]
    st = e2e[True]["stats"]
    assert st["masked_sources"] == 2 and st["masked_letters"] >= 80


def test_e2e_cli_prints_the_sessions_lines(e2e):
    base = [native.BIN_PATH, "search", "-f", e2e["db"], "-D", "0", "-y", "14", "-w", "64", "-T", "32"]
    for on in (False, True):
        out = os.path.join(e2e["tmp"], f"cli_{int(on)}.out")
        p = subprocess.run(base + (["-Z", "12,220,250", "-v"] if on else []) + [e2e["q"], out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert open(out, "rb").read() == e2e[on]["text"]
        if on:
            assert f"masked letters {e2e[True]['stats']['masked_letters']} sources 2" in p.stdout
    for bad in ("5,220,250", "12,300,200", "12", "12,220", "12,220,250,1", "12,,250", "a,220,250", "12,220,501", "33,1,2"):
        p = subprocess.run(base + ["-Z", bad, e2e["q"], os.path.join(e2e["tmp"], "bad.out")], capture_output=True, text=True)
        assert p.returncode == 1, bad
    # aln does not take it
    p = subprocess.run([native.BIN_PATH, "aln", "-Z", "12,220,250", "-i", "x", "-d", "y", "-o", os.devnull],
                       capture_output=True, text=True)
    assert "masked" not in p.stdout


# ------------------------------------------------------------------ LDS poison
@pytest.mark.parametrize("pattern", ["0xA5A5A5A5", "0x00000000"])
def test_under_lds_poison(pattern):
    """k_mask_windows stages its codes, its counts and its table in LDS: the stage-level case sets and the
    session-level record cases on the poison build, one child process per pattern."""
    here = os.path.dirname(os.path.abspath(__file__))
    poison = os.path.join(os.path.dirname(here), "ghostm_amd", "lib", "libghostm_hip_poison.so")
    assert os.path.exists(poison), "build the poison library (make -C ghostm_amd/csrc)"
    env = dict(os.environ, GHOSTM_LIB_PATH=poison, GHOSTM_LDS_POISON_PATTERN=pattern)
    p = subprocess.run([sys.executable, os.path.join(here, "mask_poison_child.py")],
                       capture_output=True, text=True, timeout=120, env=env)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, p.stderr[-3000:]
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res.get("ok") is True and res["pattern"] == pattern, (res, p.stderr[-2000:])
    assert res["sets"] == len(mc.all_case_sets()) + len(mc.carry_cases()) + 3
