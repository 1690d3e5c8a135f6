"""Child process of tests/test_gpu_read_pileup.py::test_stage_under_lds_poison
(not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_read_pileup, both instances, and k_pileup_finish<true> against the host model
on the stage sets of readpileup_cases.py: a counter that depended on LDS the
kernel never zeroed would differ under the pattern. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import readpileup_cases as rp  # noqa: E402
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
        for name, build in rp.stage_sets():
            rs = build()
            want = rp.pileup_via(rp.host_call(lib, rs), rs)
            rc.stage_setup(lib, rs)
            got = rp.pileup_via(rp.gpu_call(lib), rs)
            assert lib.FreeGpu() == 0
            rp.assert_same(got, want, name)
            hits += len(rs.src)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": hits}), flush=True)


if __name__ == "__main__":
    main()
