"""Child process of tests/test_gpu_frame_align.py::test_stage_under_lds_poison
(one process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_band_fill<true>, k_band_walk<true> and k_ops_compact against the host model on the
stage cases and the lane cases of frame_cases.py: a path that depended on LDS
the kernels never wrote would differ under one of the two patterns. Prints one
JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import frame_cases as fc  # noqa: E402
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
        builders = [b for _, b in fc.STAGE_CASES] + [lambda x=x: fc.lane_edge_case(*x) for x in fc.LANE_CASES]
        for build in builders:
            case = build()
            want = case.host()
            fc.stage_setup(lib, case)
            rec, ops = fc.gpu_frame(lib, case)
            assert lib.FreeGpu() == 0
            assert np.array_equal(rec, want[0]) and np.array_equal(ops, want[1])
            case.check(rec, ops)
            hits += len(rec)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": hits}), flush=True)


if __name__ == "__main__":
    main()
