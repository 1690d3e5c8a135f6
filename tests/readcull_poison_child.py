"""Child process of tests/test_gpu_read_cull.py::test_stage_under_lds_poison (not
a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_read_cull, every size class, against the host model on the stage cases of
readcull_cases.py: a counter or a table word the kernel read before writing it
would differ under the pattern. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import readcull_cases as cc  # noqa: E402
from ghostm_amd import native, read_cull, read_cull_host  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    hits = 0
    try:
        cases = dict(cc.shape_cases(), mixed=cc.mixed_call())
        for n in cc.SIZES:
            cases[f"size_{n}"] = cc.sized_read(n)
        for name, case in cases.items():
            cc.assert_same(read_cull(*case), read_cull_host(*case), name)
            hits += len(case[1])
        assert lib.FreeGpu() == 0
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": hits}), flush=True)


if __name__ == "__main__":
    main()
