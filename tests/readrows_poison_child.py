"""Child process of tests/test_gpu_read_rows.py::test_stage_under_lds_poison
(one process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_read_rows, both instances, against the host model on the stage sets of
readrows_cases.py: a row or a count that depended on LDS the kernel never wrote
would differ under one of the two patterns. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import readrows_cases as rc  # noqa: E402
from ghostm_amd import native  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    hits = 0
    try:
        for _, build in rc.stage_sets():
            rs = build()
            want = rs.host()
            rc.stage_setup(lib, rs)
            rec, rows = rc.gpu_rows(lib, rs)
            assert lib.FreeGpu() == 0
            assert np.array_equal(rec, want[0]) and bytes(rows) == bytes(want[1])
            hits += len(rec)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": hits}), flush=True)


if __name__ == "__main__":
    main()
