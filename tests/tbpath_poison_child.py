"""Child process of tests/test_gpu_traceback_path.py::test_stage_under_lds_poison
(one process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and makes
the stage-level check of k_tb_path_fill and k_tb_path_walk on the indel
fixture at L = 75: a path that depended on LDS the kernels never wrote would
differ from the host model under one of the two patterns. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import tbext_cases as tx  # noqa: E402
import tbpath_cases as tp  # noqa: E402
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
        L = 75
        d, chunk, tb = tx.fixture_hits(root, L)
        rec, ops = tp.stage_check(lib, d, chunk, tb, tx.blosum62(), L + 2 * 2 * 2 * 16)
        tp.assert_gapped(rec, ops)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": int(len(tb))}), flush=True)


if __name__ == "__main__":
    main()
