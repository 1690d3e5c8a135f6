"""Child process of tests/test_gpu_taxon_profile.py::test_stage_under_lds_poison
(not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code) and checks
the k_taxon_* kernels against the host model on every stage case of
taxprofile_cases.py. The kernels keep nothing in LDS, so the pattern must not
show anywhere. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import taxprofile_cases as tp  # noqa: E402
from ghostm_amd import native, set_taxonomy_gpu, taxon_profile, taxon_profile_host  # noqa: E402


def main():
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    reads = 0
    try:
        resident = None
        for name, (parent, node, min_reads) in tp.stage_cases().items():
            if parent is not resident:
                set_taxonomy_gpu(parent)
                resident = parent
            tp.assert_same(taxon_profile(node, min_reads), taxon_profile_host(parent, node, min_reads), name)
            reads += len(node)
        assert lib.FreeGpu() == 0
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "reads": reads}), flush=True)


if __name__ == "__main__":
    main()
