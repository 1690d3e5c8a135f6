"""Child process of tests/test_gpu_query_tiles.py::test_under_lds_poison (one
process per LDS pattern; not a test module itself).

Runs with GHOSTM_LIB_PATH = the LDS poison build (the tiled query formatting
kernels fill their whole LDS allocation with GHOSTM_LDS_POISON_PATTERN before
they stage their letter and codon tables) and formats the protein and DNA
record cases of tile_cases.py against the Python models: a code looked up in
LDS the kernels never wrote would differ under one of the two patterns. Prints
one JSON line."""
import json
import os
import random
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import tile_cases as tc  # noqa: E402
from ghostm_amd import native  # noqa: E402
from ghostm_amd.aligner import Session  # noqa: E402


def records(s, width):
    out, c, total = [], 0, len(s.query_lengths())
    while sum(len(x) for x in out) < total:
        out.append(s.query_records(c).reshape(-1, width))
        c += 1
    return np.concatenate(out)


def main():
    d = sys.argv[1]
    lib = native.load()
    info = (lib.GhostmBuildInfo() or b"").decode()
    pattern = os.environ.get("GHOSTM_LDS_POISON_PATTERN")
    if "LDS poison build" not in info:
        print(json.dumps({"ok": False, "error": f"not the poison build: {info}"}), flush=True)
        sys.exit(2)
    sets = 0
    try:
        with Session.for_db(["-d", os.path.join(d, "db"), "-o", os.devnull, "-D", "0"]) as s:
            for W, step in tc.PROTEIN_CASES:
                max_len = 2 * W + step + 3
                recs = tc.protein_records(W, step, max_len, random.Random(W * 1000 + step))
                want = tc.protein_tiles(recs, W, step, max_len)
                s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=W, tile_step=step, max_len=max_len)
                got = records(s, W)
                assert got.tobytes() == np.stack([tc.code_record(t[1], W) for t in want]).tobytes(), (W, step)
                assert s.query_lengths().tolist() == tc.residues(got).tolist(), (W, step)
                sets += 1
            for W, step in tc.DNA_CASES:
                recs = tc.dna_records(W, step, random.Random(W * 1000 + step))
                want = tc.dna_tiles(recs, W, step)
                s.set_queries([x[1] for x in recs], [x[0] for x in recs], width=3 * W, dna=True, tile_step=step)
                got = records(s, W)
                assert got.tobytes() == np.stack([tc.code_record(t[1], W) for t in want]).tobytes(), (W, step)
                assert s.query_lengths().tolist() == tc.residues(got).tolist(), (W, step)
                sets += 1
    except Exception:  # noqa: BLE001 (reported to the parent)
        print(json.dumps({"ok": False, "pattern": pattern, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
    print(json.dumps({"ok": True, "pattern": pattern, "sets": sets}), flush=True)


if __name__ == "__main__":
    main()
