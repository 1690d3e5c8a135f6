"""Child process of tests/test_gpu_query_mask.py::test_under_lds_poison (one
process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (k_mask_windows fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before it stages its table, its
codes and its counts) and masks the stage-level case sets, the carry cases and
the session-level record sets of mask_cases.py against the Python model: a code
or a count read from LDS the kernel never wrote would differ under one of the
two patterns. Prints one JSON line."""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import mask_cases as mc  # noqa: E402
from ghostm_amd import mask_records, native  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402


def records(s, width):
    out, c, total = [], 0, len(s.query_lengths())
    while sum(len(x) for x in out) < total:
        out.append(s.query_records(c).reshape(-1, width))
        c += 1
    return np.concatenate(out)


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    sets = 0
    try:
        for w, levels, layout in mc.all_case_sets():
            recs, srcs, step, want, counts, _ = mc.case_set(w, levels, layout)
            got, masked = mask_records(recs, layout[0], srcs, step, w, *levels)
            assert got.tobytes() == want.tobytes() and masked.tolist() == counts.tolist(), (w, levels, layout)
            sets += 1
        for name, (letters, W, step, stride, w, levels, _) in sorted(mc.carry_cases().items()):
            recs, srcs = mc.lay_out(letters, W, step, stride)
            want, counts, _ = mc.model(recs, srcs, W, step, w, *levels)
            got, masked = mask_records(recs, W, srcs, step, w, *levels)
            assert got.tobytes() == want.tobytes() and masked.tolist() == counts.tolist(), name
            sets += 1
        with Session.for_queries(["-o", os.devnull, "-D", "0"]) as s:
            for name, (seqs, names, kw, W, step) in sorted(mc.session_sets().items()):
                s.set_mask(0)
                s.set_queries(seqs, names, **kw)
                plain = records(s, W)
                srcs = mc.session_sources(s.query_tiles(), len(plain), W, kw.get("dna", False))
                want, counts, _ = mc.model(plain, srcs, W, step or W, 12, 220, 250)
                s.set_mask(12, 220, 250)
                s.set_queries(seqs, names, **kw)
                assert records(s, W).tobytes() == want.tobytes(), name
                assert s.query_masked().tolist() == counts.tolist(), name
                sets += 1
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "sets": sets}), flush=True)


if __name__ == "__main__":
    main()
