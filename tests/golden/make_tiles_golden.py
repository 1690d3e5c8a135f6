"""Regenerate the tiled-search fixture: tiles_reads.fasta and tiles_y{0,1,2}.out.

Runs only where the reference CPU program oracle/_ref/ghostm_ref has been built
(oracle/Makefile `ref`). The reads are long queries made of mutated stretches of
the protein_testset subjects (testset_db.fasta) between random flanks. The
expected text is the reference's own: its `qry -l 32` and `aln` on a FASTA that
lists every read's tiles (width 32, step 16, tests/tile_cases.starts) as
explicit records under the read's repeated name, against its own `db` of
testset_db.fasta. `ghostm search -w 32 -T 16` on the reads must print those bytes
(tests/test_gpu_query_tiles.py).

    python tests/golden/make_tiles_golden.py
"""
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tile_cases as tc  # noqa: E402

REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "ghostm_ref")
W, STEP = 32, 16


def subjects():
    out = []
    for block in open(os.path.join(HERE, "testset_db.fasta")).read().split(">")[1:]:
        name, _, seq = block.partition("\n")
        out.append("".join(seq.split()))
    return out


def make_reads():
    r = random.Random(3216)
    subs = subjects()
    rand = lambda n: "".join(r.choice(tc.AA) for _ in range(n))  # noqa: E731
    mutate = lambda s: "".join(r.choice(tc.AA) if r.random() < 0.06 else c for c in s)  # noqa: E731
    reads = []
    for i in range(24):
        sub = subs[i % len(subs)]
        a = r.randrange(0, max(len(sub) - 40, 1))
        core = mutate(sub[a:a + r.randint(30, 75)])
        reads.append((f"read{i}", rand(r.randint(0, 70)) + core + rand(r.randint(0, 60))))
    reads.append(("two_subjects", mutate(subs[0][:50]) + rand(21) + mutate(subs[2][:45])))
    reads.append(("short", mutate(subs[1][10:40])))
    reads.append(("exact_width", mutate(subs[0][5:5 + W])))
    reads.append(("no_hit", rand(97)))
    return reads


def main():
    reads = make_reads()
    with open(os.path.join(HERE, "tiles_reads.fasta"), "w") as f:
        for name, seq in reads:
            f.write(f">{name}\n{seq}\n")
    with tempfile.TemporaryDirectory() as tmp:
        tiles = os.path.join(tmp, "tiles.fa")
        with open(tiles, "w") as f:
            for t in tc.protein_tiles(reads, W, STEP):
                f.write(f">{t[0]}\n{t[1]}\n")
        q, db = os.path.join(tmp, "q"), os.path.join(tmp, "db")
        subprocess.run([REF, "qry", "-i", tiles, "-o", q, "-l", str(W)], check=True)
        subprocess.run([REF, "db", "-i", os.path.join(HERE, "testset_db.fasta"), "-o", db], check=True)
        for style in "012":
            out = os.path.join(HERE, f"tiles_y{style}.out")
            subprocess.run([REF, "aln", "-i", q, "-d", db, "-o", out, "-y", style], check=True)
            print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
