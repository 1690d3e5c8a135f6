"""Child process of tests/test_gpu_band_align.py::test_stage_under_lds_poison
(one process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_band_fill<false>, k_band_walk<false> and k_ops_compact against the host model on one stage
case (m = 2W + step + 3, B = 31, 60 hits): a path that depended on LDS the
kernels never wrote would differ under one of the two patterns. Prints one
JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import band_cases as bc  # noqa: E402
from ghostm_amd import native  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    try:
        case = bc.mixed_case(5, 2 * bc.W + bc.STEP + 3, B=31)
        want = case.host()
        bc.stage_setup(lib, case)
        rec, ops = bc.gpu_band(lib, case)
        assert lib.FreeGpu() == 0
        assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
        case.check(rec, ops)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": int(len(rec))}), flush=True)


if __name__ == "__main__":
    main()
