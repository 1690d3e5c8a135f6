"""Child process of tests/test_gpu_pileup.py::test_stage_under_lds_poison (one
process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and makes
the stage-level checks of k_pileup and k_pileup_finish: the indel fixture at
L = 75, the hand-made paths and the tile-edge shapes. A workgroup that did not
zero its own LDS histogram would add the pattern into the profile under one of
the two patterns. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pathrows_cases as pr  # noqa: E402
import pileup_cases as pc  # noqa: E402
import tbext_cases as tx  # noqa: E402
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
        d, chunk, M, qid, rec, ops = pr.fixture_paths(root, 75)
        n = pc.stage_check(lib, d, chunk, M, qid, rec, ops)
        d, chunk = pr.build_tiny(root)
        qid, rec, ops = pr.hand_paths(chunk[0], chunk[1], len(chunk[3]))
        n += pc.stage_check(lib, d, chunk, tx.blosum62(), qid, rec, ops, counts=(len(qid),), edges=True)
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "hits": int(n)}), flush=True)


if __name__ == "__main__":
    main()
