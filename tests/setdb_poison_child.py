"""Child process of tests/test_gpu_set_db.py::test_under_lds_poison (one process
per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (every kernel fills its whole
LDS allocation with GHOSTM_LDS_POISON_PATTERN before its own code; the index
kernels are built that way for this library too) and makes the kernel-level
edge set of a replaced database (every chunk length around the coding kernel's
lane, wave and workgroup widths, the subject-length, letter and X-window
records, k = 3 and 4) against the files of `ghostm db`, then syn_small's search
on a database set from FASTA against the session on the formatted files: a
table entry, a scan partial or a rank that depended on LDS the kernels never
wrote would differ under one of the two patterns. Prints one JSON line."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import setdb_cases as sd  # noqa: E402
from ghostm_amd import native  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402


def main():
    d, tmp = sys.argv[1], sys.argv[2]
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    try:
        with Session.for_queries(["-o", os.devnull, "-D", "0", "-y", "1"]) as s:
            n = sd.kernel_edge_set(s, tmp, ks=(3, 4))
        with Session(["-i", os.path.join(d, "q"), "-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as f:
            f.run()
            want = (f.output(), f.hits().tobytes())
        with Session.for_queries(["-i", os.path.join(d, "q"), "-o", os.devnull, "-D", "0"]) as s:
            s.set_db_fasta(os.path.join(d, "db.fa"))
            s.run()
            assert (s.output(), s.hits().tobytes()) == want, "syn_small: the search on the set database differs"
            hits = len(s.hits())
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "databases": n, "hits": hits}), flush=True)


if __name__ == "__main__":
    main()
