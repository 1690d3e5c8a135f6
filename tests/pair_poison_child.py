"""Child process of tests/test_gpu_pair_join.py::test_stage_under_lds_poison (not a
test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_pair_join, every size class, against the host model on the stage cases of
pair_cases.py: a staged record, a chooser word or a part of the pair's record
the kernel read before writing it would differ under the pattern. Prints one
JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pair_cases as pc  # noqa: E402
from ghostm_amd import native, pair_join, pair_join_host  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    pairs = 0
    try:
        cases = dict(pc.shape_cases(), mixed=pc.mixed_call())
        for n in pc.SIZES:
            cases[f"size_{n}"] = pc.sized_pair(n)
        for name, case in cases.items():
            pc.assert_same(pair_join(*case), pair_join_host(*case), name)
            pairs += len(case[1])
        assert lib.FreeGpu() == 0
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "pairs": pairs}), flush=True)


if __name__ == "__main__":
    main()
