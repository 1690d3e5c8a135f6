"""The adapter stage's host model (GhostmAdapterTrimHost, read_adapter.h /
read_adapter_host.cpp) against the Python model of adapter_cases.py: every
field of every record on every case set and named case, the off parameters, and
the refusals by name. No GPU."""
import os

import numpy as np
import pytest

import adapter_cases as ac
import cases
from ghostm_amd import ADAPTER_OUT_DTYPE, GhostmError, adapter_trim_host


def check_host(reads, params, filler=b"#"):
    letters, offs, lens = ac.lay_out(reads, filler)
    want, _ = ac.model_reads(reads, params)
    buf = bytearray(letters)
    out = adapter_trim_host(buf, offs, lens, *params)
    assert out.dtype == ADAPTER_OUT_DTYPE and out.tolist() == want.tolist()
    assert bytes(buf) == letters  # the letters are only read
    return out


def test_the_sets_hold_what_they_are_meant_to():
    ac.check_sets()


@pytest.mark.parametrize("m,mo,err", ac.ADAPTER_SETS)
def test_adapter_sets(m, mo, err):
    reads, adapter = ac.fixed_set(m, mo)
    check_host(reads, ac.P(adapter, b"", mo, err), adapter)
    reads, adapter = ac.random_set(m, mo, err)
    check_host(reads, ac.P(adapter, b"", mo, err), adapter)
    # the same reads with a second adapter for the odd records
    check_host(reads, ac.P(ac.adapter_of(33, 1), adapter, mo, err), adapter)


@pytest.mark.parametrize("po,err", ac.PAIR_SETS)
def test_pair_sets(po, err):
    reads = ac.random_pairs(po, err)
    check_host(reads, ac.P(b"", b"", 5, err, po), ac.TRUSEQ)
    check_host(reads, ac.P(ac.TRUSEQ, ac.TRUSEQ2, 5, err, po), ac.TRUSEQ)


@pytest.mark.parametrize("name", sorted(ac.named_cases()))
def test_named_cases(name):
    reads, params, want = ac.named_cases()[name]
    out = check_host(reads, params, params[0] or b"#")
    if want is not None:
        assert [(int(o["kept"]), int(o["adapter_at"]), int(o["pair_len"])) for o in out] == want


def read_fasta(path):
    recs = []
    for block in open(path).read().split(">")[1:]:
        lines = block.split("\n")
        recs.append((lines[0].strip(), "".join(x.strip() for x in lines[1:])))
    return recs


def test_end_to_end_reads_are_cut_where_planted():
    """The reads of the end-to-end test on the golden testset (test_gpu_read_adapter.py): the model, and the host
    model with it, finds every planted cut exactly and cuts no unplanted read."""
    single, pairs = ac.e2e_reads(dict(read_fasta(os.path.join(cases.GOLDEN, "testset_db.fasta"))))
    ac.check_e2e(single, pairs)
    for reads, params in ((single, ac.E2E_SINGLE), (pairs, ac.E2E_PAIRS)):
        out = check_host([r[1] for r in reads], params, ac.TRUSEQ)
        assert out["kept"].tolist() == [r[2] for r in reads]


def test_off_parameters_and_no_reads():
    reads = ac.random_set(33, 5, 10)[0][:40]
    out = check_host(reads, ac.P())
    assert out["kept"].tolist() == out["adapter_at"].tolist() == [len(r) for r in reads] and not out["pair_len"].any()
    assert len(check_host([], ac.P(ac.TRUSEQ))) == 0
    assert len(adapter_trim_host(b"", [], [], ac.TRUSEQ, b"", 5, 10, 20)) == 0
    # an odd count is fine while the pair rule is off, and with everything off
    check_host(reads[:3], ac.P(ac.TRUSEQ))
    assert len(adapter_trim_host(b"ACGT", [0], [4], b"", b"", 5, 10, 0)) == 1


@pytest.mark.parametrize("reason,change", ac.REFUSALS)
def test_refusals(reason, change):
    with pytest.raises(GhostmError, match="GhostmAdapterTrimHost: " + reason + ":"):
        adapter_trim_host(*ac.refusal_args(change))


def test_a_parameter_beyond_32_bits():
    with pytest.raises(GhostmError, match="param:"):
        adapter_trim_host(b"ACGT", [0], [4], b"ACGT", b"", 1 << 32, 10, 0)


def test_record_is_16_bytes():
    assert ADAPTER_OUT_DTYPE.itemsize == 16 and np.dtype(ac.OUT_DTYPE) == ADAPTER_OUT_DTYPE
