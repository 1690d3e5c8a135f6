"""Child process of tests/test_gpu_dp_edges.py::test_layout_sweep_under_lds_poison
(one process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and makes
the default-form layout sweep of dp_cases.py: K1's candidates, K2's scores and
ends and K3's tracebacks at both ends of every layout range against the model
results the parent saved. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dp_cases as dp  # noqa: E402
from ghostm_amd import native  # noqa: E402


def main():
    root = sys.argv[1]
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    try:
        dp.load_models(root)
        ncand, nhits = dp.layout_sweep(root, dp.WIDTHS)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "candidates": int(ncand), "hits": int(nhits)}), flush=True)


if __name__ == "__main__":
    main()
