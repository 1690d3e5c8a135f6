"""The host model of the quality stage (GhostmQualityTrimHost,
ghostm_amd/csrc/read_quality_host.cpp) against the Python model of
qual_cases.py on every case set and named case, its refusals, and the asserts
on what the sets hold. No device."""
import ctypes

import numpy as np
import pytest

import qual_cases as qc
from ghostm_amd import GhostmError, QUAL_OUT_DTYPE, native, quality_trim_host


def test_sets_hold_what_they_are_meant_to():
    qc.check_sets()
    assert QUAL_OUT_DTYPE == qc.OUT_DTYPE and ctypes.sizeof(native.GhostmQualOut) == 16


def check_host(reads, params):
    letters, qual, offs, lens = qc.lay_out(reads)
    want, want_out, _ = qc.model(letters, qual, offs, lens, params)
    got, out = quality_trim_host(letters, qual, offs, lens, *params)
    assert out.tolist() == want_out.tolist()
    assert got == want and qc.gaps_untouched(got, offs, lens)
    return out


@pytest.mark.parametrize("params", qc.PARAM_SETS)
def test_host_equals_model_on_the_random_sets(built, params):
    check_host(qc.random_set(params)[0], params)


@pytest.mark.parametrize("name", sorted(qc.carry_cases()))
def test_host_equals_model_on_the_named_cases(built, name):
    reads, params, check = qc.carry_cases()[name]
    check(check_host(reads, params))


def test_off_reads_no_quality(built):
    reads = [(b"ACGT", b"\x00\xff  "), (b"", b"")]
    letters, qual, offs, lens = qc.lay_out(reads)
    got, out = quality_trim_host(letters, qual, offs, lens, 0, 0, 0)
    assert got == letters and out.tolist() == [(0, 4, 0, 0), (0, 0, 0, 0)]
    got, out = quality_trim_host(b"", b"", [], [], 20, 0, 0)
    assert got == b"" and len(out) == 0


REFUSALS = [
    ("param", dict(trim=94)), ("param", dict(mask=94)), ("param", dict(min_len=(1 << 24) + 1)),
    ("record", dict(offsets=[0, 99])), ("record", dict(lengths=[4, 95])), ("record", dict(offsets=[0, 1 << 40])),
    ("length", dict(big=True)),
]


def refusal_args(change):
    """(letters, qual, offsets, lengths, trim, mask, min_len) with one thing wrong"""
    if change.get("big"):  # a read of 2^24 + 1 letters inside the buffer
        n = (1 << 24) + 1
        return b"A" * n, b"I" * n, [0], [n], 20, 0, 0
    letters, qual = b"ACGT" * 25, b"I" * 100
    return (letters, qual, change.get("offsets", [0, 50]), change.get("lengths", [4, 50]), change.get("trim", 20),
            change.get("mask", 0), change.get("min_len", 0))


@pytest.mark.parametrize("reason,change", REFUSALS)
def test_host_refusals(built, reason, change):
    with pytest.raises(GhostmError, match="GhostmQualityTrimHost: " + reason + ":"):
        quality_trim_host(*refusal_args(change))


def test_host_null_refusal_and_ranges_accepted(built):
    lib = native.load()
    lens = np.array([4], dtype=np.uint32)
    out = np.zeros(1, dtype=QUAL_OUT_DTYPE)
    rc = lib.GhostmQualityTrimHost(None, None, 4, None, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 1, 20, 0, 0,
                                   out.ctypes.data_as(ctypes.POINTER(native.GhostmQualOut)))
    assert rc == 1 and "null:" in native.last_error()
    # the ranges' last values pass; min_len over the read fails it and leaves its letters
    got, out = quality_trim_host(b"ACGT", b"IIII", [0], [4], 93, 93, 1 << 24)
    assert got == b"ACGT" and out.tolist() == [(0, 0, 0, 0)]
