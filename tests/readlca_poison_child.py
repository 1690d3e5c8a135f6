"""Child process of tests/test_gpu_read_lca.py::test_stage_under_lds_poison (not a
test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
k_read_lca_wave and k_read_lca, every size class, against the host model on the
stage cases of readlca_cases.py: a counter, a table slot or a staged candidate
the kernel read before writing it would differ under the pattern. Prints one
JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import readlca_cases as lc  # noqa: E402
from ghostm_amd import native, read_lca, read_lca_host, set_taxonomy_gpu  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    reads = 0
    try:
        cases = dict(lc.shape_cases(), mixed=lc.mixed_call())
        cases.update(lc.tree_cases())
        for n in lc.SIZES:
            cases[f"size_{n}"] = lc.sized_read(n)
        resident = None
        for name, case in cases.items():
            if case[0] is not resident:
                set_taxonomy_gpu(case[0])
                resident = case[0]
            lc.assert_same(read_lca(*case[1:]), read_lca_host(*case), name)
            reads += len(case[1]) - 1
        assert lib.FreeGpu() == 0
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "reads": reads}), flush=True)


if __name__ == "__main__":
    main()
