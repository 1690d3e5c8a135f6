"""The read-level cull on the host (GhostmReadCullHost, no device): against the
brute-force model of readcull_cases.py (per-position counters, a plain sorted
loop; no code shared with read_cull.h) on the small shapes, the reads at the
kernel's class borders, one call that mixes them and a few hundred random reads
with coordinates below 2000; every refusal with the outputs untouched; the
struct layouts and the new symbols; the segment arithmetic as a stand-alone
program, plain and under -fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import readcull_cases as cc
from ghostm_amd import CULL_HIT_DTYPE, CULL_OUT_DTYPE, GhostmError, native, read_cull_host

SRC = os.path.join(os.path.dirname(__file__), "native", "test_read_cull.cpp")
SHAPES = cc.shape_cases()


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_equals_the_model_on_the_shapes(name):
    case = SHAPES[name]
    want = cc.model(*case)
    cc.expected_shapes(name, want)
    cc.assert_same(read_cull_host(*case), want, name)


@pytest.mark.parametrize("n", cc.SIZES)
def test_host_equals_the_model_at_the_class_borders(n):
    case = cc.sized_read(n)
    want = cc.model(*case)
    st = want["status"]
    assert (st == 0).sum() > n // 8 and (st == 1).sum() and (st == 2).sum() and (st == 3).sum(), np.bincount(st)
    assert sorted(want["order"].tolist()) == list(range(n))
    cc.assert_same(read_cull_host(*case), want, n)


def test_host_equals_the_model_on_the_mixed_call():
    case = cc.mixed_call()
    cc.assert_same(read_cull_host(*case), cc.model(*case), "mixed")


def test_host_equals_the_model_on_random_reads():
    reads = 0
    seen = np.zeros(4, dtype=np.int64)
    for k, case in enumerate(cc.random_calls(150)):
        want = cc.model(*case)
        cc.assert_same(read_cull_host(*case), want, ("random", k))
        reads += len(case[0]) - 1
        seen += np.bincount(want["status"], minlength=4)
    assert reads >= 300 and (seen > 100).all(), (reads, seen)


def test_hits_outside_every_read_get_no_record():
    _, h, k, pct = SHAPES["nested"]
    rb = np.array([1, 3], dtype=np.uint32)
    out = np.full(4 * len(h), 0x5A5A5A5A, dtype=np.uint32).view(CULL_OUT_DTYPE)
    read_cull_host(rb, h, k, pct, out=out)
    assert out[0].tolist() == (0x5A5A5A5A,) * 4
    cc.assert_same(out[1:], cc.model(rb, h, k, pct)[1:], "inner read")


def test_host_refusals():
    cc.check_refusals("GhostmReadCullHost")
    with pytest.raises(GhostmError, match="param"):
        read_cull_host(*SHAPES["nested"][:2], top_k=0)


def test_struct_layout_and_symbols():
    assert ctypes.sizeof(native.GhostmCullHit) == CULL_HIT_DTYPE.itemsize == 24
    assert ctypes.sizeof(native.GhostmCullOut) == CULL_OUT_DTYPE.itemsize == 16
    for struct, dtype in ((native.GhostmCullHit, CULL_HIT_DTYPE), (native.GhostmCullOut, CULL_OUT_DTYPE)):
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name
    assert [n for n, _ in native.GhostmReadCullStats._fields_] == [
        "seconds_cull", "cull_launches", "cull_reads", "cull_hits", "cull_kept", "cull_dups", "cull_culled"]
    assert ctypes.sizeof(native.GhostmReadCullStats) == 56
    stats = [n for n, _ in native.GhostmStats._fields_]   # GhostmStats keeps its layout
    assert stats[-5:] == ["seconds_pileup", "pileup_launches", "pileup_windows", "pileup_parts", "pileup_columns"]
    lib = native.load()
    for sym in ("ReadCullGpu", "GhostmReadCullHost", "GhostmStageReadCullStats"):
        assert hasattr(lib, sym) and sym in native.SIGNATURES, sym
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ghostm_hip.h")).read()
    for sym in ("ReadCullGpu(", "GhostmReadCullHost(", "GhostmStageReadCullStats(", "GhostmCullHit;", "GhostmCullOut;",
                "GhostmReadCullStats;"):
        assert sym in header, sym


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_segment_arithmetic_native(flags, tmp_path):
    exe = str(tmp_path / "test_read_cull")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "trials ok" in r.stdout
