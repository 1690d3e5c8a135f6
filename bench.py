"""Benchmark of the `aln` hot path (BASELINE.json metric: query residues aligned/s,
bit-identical hits). Workload = BASELINE.json configs[3] (cfg4): synthetic 1M
queries (avg ~265 aa before the 127-residue cap, L = 127) against a 10M-residue
DB, default `aln` options (BLOSUM62 11/1, -b 10, -r 16, -t 2, -s 2).

    python bench.py [--gpus N --steps K --warmup W] [--preset cfg4|cfg3|cfg5|cfg2]
                    [--queries N] [--dump-outputs DIR]
                    [--full [--cpu-sample 10000] [--cpu-sample-all 16000] [--no-cpu] [--no-e2e]]

A plain run does what the headline figure needs and no more: it builds the
inputs, opens the session, warms up, times the K steps, compares the last step's
whole output with the reference pin, writes --dump-outputs and prints the line.
`--full` adds the legs that take runs of their own: the warm and cold end-to-end
runs, the two CPU baselines and, at N > 1, rank 0's unsharded comparison run
(`--no-e2e` / `--no-cpu` drop single legs of a full run).

`--dump-outputs DIR` writes what the last timed step returned to its caller as
DIR/<name>.npy (float64 / float32, see dump_outputs). The inputs are a function
of the arguments alone, so two builds can be compared output for output.

A step = one full `aln` pass over the rank's query shard with inputs resident in
HBM: K1 seed -> K2 score -> K4 merge -> K3 traceback -> E-values + text
formatting (in memory) -> (N > 1) the one RCCL gather of the 32-byte hit records
to rank 0.

Multi-GPU (north_star: "shard the query batch across the 8 GPUs ... single RCCL
gather"): one process per GPU. `--gpus N` without WORLD_SIZE starts the N ranks
itself (ghostm_amd/launch.py: children spawned before any GPU call, rank 0's
line forwarded); under torchrun WORLD_SIZE must equal --gpus. ONE query set is
cut into N balanced, name-group-aligned shards (GhostmSessionCreateShardEx);
each rank searches its shard against a full DB replica, so total work is fixed
as N grows ("strong"). Each rank is pinned to its GPU's NUMA-local CPUs. A step
ends with one MIN all-reduce of every rank's ok flag (one rank's failure stops
all ranks) and the one data-path collective: a gather of fixed-capacity hit
record buffers with a count header. After the timed steps every rank writes its
text at its offset of one output file, and rank 0 checks the assembled file
against the reference pin (and, with --full, against an unsharded run).

Parity in the line: `full_output_matches_reference` compares the sha256 of the
whole output of the last timed step (N = 1) or of the assembled file (N > 1) with
the reference CPU program's output for the same full workload
(tests/golden/full_golden.json). A mismatch (or, with --full, a CPU-sample or
end-to-end file mismatch) nulls `value` and exits non-zero.
"""
from __future__ import annotations

import argparse
import datetime
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from ghostm_amd import launch, workloads  # noqa: E402

PEAK_VALU_TOPS = 78.6   # 256 CU x 4 SIMD x 32 lanes/cycle x 2.4 GHz int32 ops (MI355X_MICROARCH.md)
PEAK_VALU_PK16_TOPS = 157.3  # the same issue rate, two 16-bit ops per lane (v_pk_*)
PEAK_HBM_GBS = 8000.0   # HBM3E spec
SCORE_OPS_PER_CELL = 10  # Gotoh cell: add, max3 (H), add (open), add+max (E), add+max (F), max (colmax)
TB_OPS_PER_CELL = 20     # traceback cell with match/length bookkeeping
FULL_GOLDEN = os.path.join(REPO, "tests", "golden", "full_golden.json")
VALU_ISSUE = os.path.join(REPO, "profiles", "r2_valu_issue.json")
PMC = os.path.join(REPO, "profiles", "pmc_traffic.json")  # cfg4; other presets: pmc_traffic_<preset>.json
ISA_MIX = os.path.join(REPO, "profiles", "r3_k2_isa_mix.json")  # k_score16f<32, true> (16-bit profile rows)
ISA_MIX_UNIT = os.path.join(REPO, "profiles", "r6_k2_unit_isa_mix.json")  # k_score16f<32, true, true> (unit-pair words, round 6)
ISA_MIX_PAIR = os.path.join(REPO, "profiles", "r5_k2_pair_isa_mix.json")  # k_score_pair<32> (pair table)
VOP2_IN_MIX_CYCLES = 3.44  # fast VOP2 add inside a 1:2 pk_max3:add stream (profiles/r2c_valu_issue_pmc.txt)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_data(root: str, preset: str, nq: int) -> tuple[str, str]:
    db = workloads.make_db(preset, os.path.join(root, "db"))
    q = workloads.make_queries(preset, os.path.join(root, "q"), 0, nq)
    return q, db


def _exe():
    ref = os.path.join(REPO, "oracle", "_ref", "ghostm_ref")
    port = os.path.join(REPO, "oracle", "_build", "ghostm_oracle")
    return (ref, "reference") if os.path.exists(ref) else (port, "port")


def _gpu_text(q: str, db: str, aln: list) -> tuple[bytes, int]:
    from ghostm_amd.aligner import Session

    with Session(["-i", q, "-d", db, "-o", os.devnull, "-D", str(_device())] + aln) as s:
        s.run()
        return s.output(), s.stats()["query_residues"]


def _wait(procs: list, label: str) -> list:
    """Wait for the CPU baseline processes, logging progress every 30 s (a long
    silent wait reads as a hung job to the GPU harness)."""
    t0 = time.perf_counter()
    while any(p.poll() is None for p in procs):
        try:
            next(p for p in procs if p.poll() is None).wait(timeout=30)
        except subprocess.TimeoutExpired:
            log(f"[cpu] {label}: {time.perf_counter() - t0:.0f} s")
    return [p.returncode for p in procs]


def cpu_baseline(root: str, preset: str, db: str, nsample: int, aln: list) -> dict:
    """The reference's own CPU path (oracle/_ref/ghostm_ref: GHOSTM's aligner.cpp
    compiled from the reference sources, run without -D; this repo's restatement
    oracle/ghostm_oracle where the reference build is absent) on the first
    `nsample` queries of the workload, single-threaded as the reference is. The
    GPU output on the same sample must be byte-identical."""
    exe, kind = _exe()
    q = workloads.make_queries(preset, os.path.join(root, "cpu1"), 0, nsample)
    out = os.path.join(root, "cpu1", "cpu.out")
    t0 = time.perf_counter()
    p = subprocess.Popen([exe, "aln", "-i", q, "-d", db, "-o", out] + aln,
                         stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if _wait([p], f"1-core reference on {nsample} queries")[0] != 0:
        raise RuntimeError("CPU baseline failed")
    dt = time.perf_counter() - t0
    gpu, residues = _gpu_text(q, db, aln)
    same = gpu == open(out, "rb").read()
    what = ("reference aligner.cpp CPU path (oracle/_ref/ghostm_ref, reference sources, g++ -O2)"
            if kind == "reference" else "CPU restatement (oracle/ghostm_oracle.cpp, g++ -O2)")
    return {"value": residues / dt, "unit": "query residues/s", "cores": 1, "kind": kind,
            "sample": f"first {nsample} queries of the workload vs the same DB ({residues} residues, "
                      f"{dt:.1f} s incl. the process's file loads, {what}, 1 thread)",
            "bit_identical_to_gpu_on_sample": bool(same)}


def reference_split(root: str, preset: str, db: str, nsample: int, aln: list, procs: int):
    """The CPU program (reference build, else the restatement) over the first
    `nsample` queries as `procs` concurrent processes on contiguous query ranges.
    Returns (concatenated output, wall seconds, processes, queries per process),
    or None if a process failed."""
    exe, _ = _exe()
    per = (nsample + procs - 1) // procs
    parts = []
    for k in range(procs):
        n = min(per, nsample - k * per)
        if n <= 0:
            break
        d = os.path.join(root, f"part{k}")
        parts.append((workloads.make_queries(preset, d, k * per, n), d))
    t0 = time.perf_counter()
    running = [subprocess.Popen([exe, "aln", "-i", q, "-d", db, "-o", f"{d}/cpu.out"] + aln,
                                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for q, d in parts]
    rcs = _wait(running, f"{len(running)}-process reference on {nsample} queries")
    dt = time.perf_counter() - t0
    if any(rcs):
        return None
    return b"".join(open(f"{d}/cpu.out", "rb").read() for _, d in parts), dt, len(parts), per


def cpu_baseline_all_cores(root: str, preset: str, db: str, nsample: int, aln: list) -> dict | None:
    """SURVEY §8 d4's second CPU figure: the reference on all host cores the job
    may use, as one process per core over contiguous query ranges (the reference
    is single-threaded; queries are independent). The concatenated outputs must
    equal the GPU output on the same sample."""
    exe, kind = _exe()
    # the box's CPU share is 16 (OMP_NUM_THREADS is set to it); os.cpu_count()
    # there reports the whole machine
    procs = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)), os.cpu_count() or 1))
    split = reference_split(os.path.join(root, "cpuN"), preset, db, nsample, aln, procs)
    if split is None:
        return None
    joined, dt, nparts, per = split
    q = workloads.make_queries(preset, os.path.join(root, "cpuN", "all"), 0, nsample)
    gpu, residues = _gpu_text(q, db, aln)
    return {"value": residues / dt, "unit": "query residues/s", "cores": nparts, "kind": kind,
            "sample": f"first {nsample} queries as {nparts} processes over contiguous query ranges "
                      f"({per} each, {dt:.1f} s incl. each process's file loads)",
            "bit_identical_to_gpu_on_sample": joined == gpu}


def _device() -> int:
    # GHOSTM_BENCH_DEVICE pins every rank to one device (rehearsing the
    # multi-rank path on a one-GPU machine)
    return int(os.environ.get("GHOSTM_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def _json(path: str) -> dict | None:
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    return None


def _sha_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def write_assembled(dist, coll_dev, rank: int, world: int, path: str, text: bytes) -> None:
    """Every rank writes its text at its offset of the one output file (rank
    order = the unsharded order); rank 0 creates it at its final size first."""
    import torch

    n = torch.tensor([len(text)], device=coll_dev, dtype=torch.int64)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    off = sum(int(x.item()) for x in sizes[:rank])
    if rank == 0:
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.ftruncate(fd, sum(int(x.item()) for x in sizes))
        os.close(fd)
    dist.barrier()
    fd = os.open(path, os.O_WRONLY)
    try:
        view = memoryview(text)
        while view:
            w = os.pwrite(fd, view, off)
            view, off = view[w:], off + w
    finally:
        os.close(fd)
    dist.barrier()


DUMP_HIT_ROWS = 300_000    # x (8 fields + the row index) x float64 = 21.6 MB
DUMP_TEXT_BYTES = 2_000_000  # x (float32 byte + float64 offset) = 24 MB


def dump_outputs(out_dir: str, text: bytes, hits) -> None:
    """What the last timed step handed its caller, as .npy arrays (float64 / float32,
    under 46 MB in all, below the 64 MB a dump may take):

      hits.npy              [rows, 8] float64: the hit records (HIT_DTYPE fields in
                            order; the u32 fields are exact in float64). All of
                            them, or the rows hits_rows.npy names.
      hits_rows.npy         [rows] float64: the record index of each row of hits.npy
                            (a fixed seeded sample, ascending, once there are more
                            than DUMP_HIT_ROWS records)
      hits_count.npy        [1] float64: records in all
      output_text.npy       [n] float32: the output text's bytes at the offsets
                            output_text_offsets.npy names (all of it, or a fixed
                            seeded sample of DUMP_TEXT_BYTES offsets, ascending)
      output_text_offsets.npy  [n] float64
      output_bytes.npy      [1] float64: length of the whole text
      output_sha256.npy     [32] float32: the sha256 digest of the whole text, one
                            byte per element

    N > 1: the records are the gathered ones (all ranks, rank order), the text is
    rank 0's shard."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(20240607)
    n = len(hits)
    rows = np.arange(n) if n <= DUMP_HIT_ROWS else np.sort(rng.choice(n, DUMP_HIT_ROWS, replace=False))
    picked = hits[rows]
    table = np.empty((len(rows), len(hits.dtype.names)), dtype=np.float64)
    for j, name in enumerate(hits.dtype.names):
        table[:, j] = picked[name]
    raw = np.frombuffer(text, dtype=np.uint8)
    offs = (np.arange(len(raw)) if len(raw) <= DUMP_TEXT_BYTES
            else np.sort(rng.choice(len(raw), DUMP_TEXT_BYTES, replace=False)))
    digest = np.frombuffer(hashlib.sha256(text).digest(), dtype=np.uint8)
    for name, arr in (("hits", table), ("hits_rows", rows.astype(np.float64)),
                      ("hits_count", np.array([n], dtype=np.float64)),
                      ("output_text", raw[offs].astype(np.float32)),
                      ("output_text_offsets", offs.astype(np.float64)),
                      ("output_bytes", np.array([len(raw)], dtype=np.float64)),
                      ("output_sha256", digest.astype(np.float32))):
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def full_pin(preset: str, nq: int, aln: list) -> dict | None:
    """The reference pin for this exact workload, if it is the full preset."""
    pins = _json(FULL_GOLDEN) or {}
    pin = pins.get(preset)
    w = workloads.WORKLOADS[preset]
    if not isinstance(pin, dict) or nq != w["queries"] or aln != w["aln"]:
        return None
    return pin


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one process per GPU); without WORLD_SIZE, N > 1 starts them itself")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", choices=sorted(workloads.WORKLOADS), default="cfg4",
                    help="BASELINE.json config (cfg4 = the headline workload)")
    ap.add_argument("--queries", type=int, default=None, help="queries of the whole job (default: preset)")
    ap.add_argument("--cpu-sample", type=int, default=None,
                    help="queries of the 1-core CPU baseline (default 10000; cfg5 4000)")
    ap.add_argument("--cpu-sample-all", type=int, default=None,
                    help="queries of the all-cores CPU baseline (default 16000; cfg5 8000)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs that take runs of their own: warm and cold end to end, the CPU "
                         "baselines, (N > 1) the unsharded comparison run")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the end-to-end legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--aln", default="", help="extra aln options appended to the preset's (e.g. '-l 16')")
    args = ap.parse_args()
    # before anything touches the GPU: launch the ranks ourselves, or check
    # that torchrun's world is the one asked for
    world, spawn = launch.world_from_env(args.gpus)
    if spawn:
        sys.exit(launch.spawn([os.path.abspath(__file__)] + sys.argv[1:], world))
    preset = args.preset
    w = workloads.WORKLOADS[preset]
    nq = args.queries or w["queries"]
    aln_args = list(w["aln"]) + args.aln.split()

    rank = int(os.environ.get("RANK", "0"))
    dist = None
    coll_dev = None
    placement = None
    # GHOSTM_BENCH_DIST=1 takes the collective path at world 1 too (under
    # torchrun --nproc-per-node 1): RCCL init, the record gather, the reductions
    if world > 1 or os.environ.get("GHOSTM_BENCH_DIST") == "1":
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(_device())
        # RCCL ("nccl") over xGMI; GHOSTM_BENCH_BACKEND=gloo rehearses the same
        # calls on a one-GPU machine (RCCL refuses two ranks on one device)
        backend = os.environ.get("GHOSTM_BENCH_BACKEND", "nccl")
        # a rank that never arrives ends the job instead of hanging it
        timeout = datetime.timedelta(seconds=float(os.environ.get("GHOSTM_BENCH_PG_TIMEOUT", "900")))
        # the backends' own connection messages (gloo prints its peer mesh on
        # stdout) go to stderr: stdout carries only rank 0's JSON line
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        try:
            if backend == "nccl":
                dist.init_process_group(backend, device_id=torch.device("cuda", _device()), timeout=timeout)
            else:
                dist.init_process_group(backend, timeout=timeout)
        finally:
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
        coll_dev = "cuda" if backend == "nccl" else "cpu"
        if os.environ.get("GHOSTM_BENCH_NO_BIND") != "1":
            placement = launch.bind_numa(dist, rank, _device())
    from ghostm_amd.aligner import HIT_DTYPE, Session

    # one data set for the whole job, built by rank 0 (ranks share the host)
    if args.workdir:
        workdir = args.workdir
    elif world > 1:
        workdir = os.path.join(tempfile.gettempdir(), f"ghostm_bench_{os.environ.get('MASTER_PORT', '0')}")
    else:
        workdir = tempfile.mkdtemp(prefix="ghostm_bench_")
    t0 = time.perf_counter()
    if rank == 0:
        qprefix, dbprefix = make_data(workdir, preset, nq)
        log(f"[rank 0] data ready in {time.perf_counter() - t0:.1f}s at {workdir}")
    if dist is not None:
        dist.barrier()
    qprefix, dbprefix = os.path.join(workdir, "q", "q"), os.path.join(workdir, "db", "db")
    out_path = os.path.join(workdir, "out")
    argv = ["-i", qprefix, "-d", dbprefix, "-o", out_path, "-D", str(_device())] + aln_args

    def open_session():
        """N > 1: a rank-local shard session (reads and counts only its own
        queries; the ranks agree on the unsharded batch plan with one all-gather
        of candidate totals at creation, GhostmSessionCreateShardEx)."""
        if world == 1:
            return Session(argv)
        from ghostm_amd.shard import torch_allgather

        return Session(argv, shard=(rank, world), exchange=torch_allgather(dist, device=coll_dev))

    def guarded(fn, what):
        """fn() on every rank, then one ok-flag all-reduce: any rank's failure
        raises on every rank (its own error on the failing one)."""
        if dist is None:
            return fn()
        try:
            out = fn()
        except BaseException:
            launch.agree(dist, False, coll_dev, what)
            raise
        launch.agree(dist, True, coll_dev, what)
        return out

    sess = guarded(open_session, "session create")
    if os.environ.get("GHOSTM_BENCH_PAUSE_S"):  # diagnostics: idle time between create and the first run
        time.sleep(float(os.environ["GHOSTM_BENCH_PAUSE_S"]))
    gatherer = None
    if dist is not None:
        import torch

        from ghostm_amd.shard import RecordGather

        # fixed capacity: the most records any shard's run can return, as the
        # library bounds it (its name groups x max(-b, 1), GhostmSessionHitCapacity)
        cap = torch.tensor([sess.hit_capacity()], device=coll_dev, dtype=torch.int64)
        dist.all_reduce(cap, op=dist.ReduceOp.MAX)
        gatherer = RecordGather(dist, int(cap.item()), HIT_DTYPE.itemsize, coll_dev)
    fills = {"device_hits_into": 0, "device_hits_copy": 0}  # which fill branch the steps took

    def fill():
        """The gather payload from the last run's device records."""
        if coll_dev == "cuda":  # RCCL: the library copies straight into the gather buffer
            n = sess.device_hits_into(gatherer.payload(), gatherer.cap)
            fills["device_hits_into"] += 1
        else:  # gloo rehearsal: the records still leave the GPU by a device copy
            recs = sess.device_hits()
            n = recs.numel() // HIT_DTYPE.itemsize
            if n > gatherer.cap:
                raise ValueError(f"{n} hit records exceed the gather capacity {gatherer.cap}")
            gatherer.payload()[: recs.numel()].copy_(recs)
            fills["device_hits_copy"] += 1
        gatherer.set_count(n)

    def step():
        guarded(sess.run, "run")
        if gatherer is not None:
            # a failing fill (capacity, copy) stops every rank here, not in the gather
            guarded(fill, "gather fill")
            # the single data-path collective: hit records to rank 0
            gatherer.gather()

    for _ in range(args.warmup):
        step()

    def sync():
        if dist is not None:
            import torch

            dist.barrier()
            torch.cuda.synchronize()

    sync()
    t = time.perf_counter()
    st_acc = None
    step_ms = []  # per-step host wall time of this rank (the first shows any one-time stall)
    for _ in range(args.steps):
        ts = time.perf_counter()
        step()
        step_ms.append((time.perf_counter() - ts) * 1e3)
        st = sess.stats()
        if st_acc is None:
            st_acc = {k: 0 for k in st}
        for k, v in st.items():
            st_acc[k] += v
    sync()
    elapsed = local_elapsed = time.perf_counter() - t
    per_rank = None
    physical = 1
    if dist is not None:
        import torch

        e = torch.tensor([elapsed], device=coll_dev, dtype=torch.float64)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())
        res = torch.tensor([st_acc["query_residues"]], device=coll_dev, dtype=torch.float64)
        dist.all_reduce(res)
        total_res = float(res.item())
        # each rank's step breakdown, and the GPUs the ranks actually ran on
        mine = {"rank": rank, "device": _device(), "host": os.uname().nodename, "placement": placement,
                "ms_per_step_local": local_elapsed / args.steps * 1e3,
                **{k: st_acc[k] / args.steps for k in ("queries", "query_residues", "candidates", "hits")},
                **{k.replace("seconds_", "ms_"): st_acc[k] / args.steps * 1e3
                   for k in ("seconds_total", "seconds_seed", "seconds_score", "seconds_traceback",
                             "seconds_merge", "seconds_output")}}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
        physical = len({(r["host"], r["device"]) for r in per_rank})
    else:
        total_res = float(st_acc["query_residues"])

    # ---- parity of the timed workload's whole output (last timed step)
    pin = full_pin(preset, nq, aln_args)
    text = sess.output()
    matches = None
    gather_check = None
    timed_sha = None  # rank 0: sha256 of the timed run's whole output
    if args.dump_outputs and rank == 0:
        recs = sess.hits()
        if gatherer is not None:
            import numpy as np

            recs = np.concatenate([m.cpu().numpy().view(HIT_DTYPE) for m in gatherer.records()])
        dump_outputs(args.dump_outputs, text, recs)
        del recs
    if dist is None:
        timed_sha = hashlib.sha256(text).hexdigest()
        if pin:
            matches = len(text) == pin["bytes"] and timed_sha == pin["sha256"]
    elif not args.full:  # the assembled file against the reference pin, no run of its own
        if pin:
            write_assembled(dist, coll_dev, rank, world, out_path, text)
            if rank == 0:
                matches = os.path.getsize(out_path) == pin["bytes"] and _sha_file(out_path) == pin["sha256"]
    else:  # also at world 1 under GHOSTM_BENCH_DIST=1: the gather path checks itself
        write_assembled(dist, coll_dev, rank, world, out_path, text)
        # rank 0 checks the last step's gather (the one collective) and the
        # assembled file against an unsharded run of the same queries on its
        # GPU, and the file against the reference pin when one applies
        import torch

        hits = torch.tensor([sess.stats()["hits"]], device=coll_dev, dtype=torch.int64)
        dist.all_reduce(hits)
        if rank == 0:
            gathered = b"".join(m.cpu().numpy().tobytes() for m in gatherer.records())
            with Session(argv) as whole:
                whole.run()
                want_rec = whole.hits().tobytes()
                want_text = whole.output()
            file_sha = timed_sha = _sha_file(out_path)
            gather_check = {
                "records_gathered": len(gathered) // HIT_DTYPE.itemsize,
                "records_equal_summed_hits": len(gathered) // HIT_DTYPE.itemsize == int(hits.item()),
                "gathered_records_equal_unsharded": gathered == want_rec,
                "assembled_file_equals_unsharded": file_sha == hashlib.sha256(want_text).hexdigest(),
                "records_nonempty": len(gathered) > 0,
            }
            ok_gather = all(v for k, v in gather_check.items() if k != "records_gathered")
            if pin:
                matches = (os.path.getsize(out_path) == pin["bytes"] and file_sha == pin["sha256"]
                           and ok_gather)
            else:
                matches = ok_gather
            del want_text, want_rec, gathered
        dist.barrier()
    del text

    # ---- end to end: create (file loads + H2D), run, write the output file;
    # the median of five runs, each file checked (the output write into the
    # page cache stalls now and then: single runs of cfg3 spread from 33 to 49
    # ms, profiles/r4n_e2e/)
    e2e = None
    if args.full and not args.no_e2e:
        runs, files_ok, create_s = [], [], []
        for _ in range(5):
            # a fresh output path per run (truncating the last run's 0.5 GB file
            # would free its page-cache pages inside the timed region)
            if rank == 0 and os.path.exists(out_path):
                os.remove(out_path)
            # every run starts with the previous run's dirty output pages written
            # back and a second to settle, untimed (otherwise that writeback slowed
            # the next run's writes and reads: cfg3 runs took 37, 44 and 53 ms in
            # a row, profiles/r4l_e2e/). The inputs stay in the page cache: the
            # file loads are warm-cache reads, as for any repeated search of a DB
            os.sync()
            time.sleep(float(os.environ.get("GHOSTM_BENCH_SETTLE_S", "1.0")))
            if dist is not None:
                dist.barrier()
            te = time.perf_counter()
            with guarded(open_session, "end-to-end session create") as s2:
                create_s.append(time.perf_counter() - te)
                if world == 1:
                    s2.run(to_file=True)  # the output file is written while the search runs
                else:
                    guarded(s2.run, "end-to-end run")
                    write_assembled(dist, coll_dev, rank, world, out_path, s2.output())
                # the output file is complete here; the session's teardown (device
                # frees) is not part of the job, as at process exit
                dt = time.perf_counter() - te
                e2e_res = s2.stats()["query_residues"]
            if dist is not None:
                import torch

                v = torch.tensor([dt, e2e_res], device=coll_dev, dtype=torch.float64)
                mx = v.clone()
                dist.all_reduce(mx, op=dist.ReduceOp.MAX)
                dist.all_reduce(v)
                dt, e2e_res = float(mx[0].item()), float(v[1].item())
            runs.append((dt, e2e_res))
            if rank == 0:  # the file this run wrote: the reference pin, else the timed run's output
                sha = _sha_file(out_path)
                files_ok.append(sha == (pin["sha256"] if pin else timed_sha))
        dt, e2e_res = sorted(runs)[len(runs) // 2]
        e2e = {"seconds": dt, "value": e2e_res / dt, "unit": "query residues/s", "runs_s": [r[0] for r in runs],
               "statistic": f"median of {len(runs)}", "kind": "warm, in-process",
               "create_s": create_s,  # this rank's session create per run (file loads, H2D)
               "includes": "session create (query/DB/index file loads from a warm page cache, dirty pages written "
                           "back first; H2D; N > 1: rank-local reads and the "
                           "batch-plan all-gather), the search, text formatting and the output file write "
                           "(N = 1: written while the search runs; N > 1: every rank writes its slice of the "
                           "one file); sessions run one after another in this process, which keeps device "
                           "blocks from the previous session (DevPool)"}
        if rank == 0:
            e2e["output_files_match_reference" if pin else "output_files_match_timed_run"] = all(files_ok)
            if not all(files_ok):
                matches = False

    # ---- end to end, cold: the `ghostm aln` command itself in a fresh process
    # (HIP runtime start, file loads, H2D, search, the output file; no device
    # blocks from an earlier session), spawn to exit, the median of three
    e2e_cold = None
    if args.full and not args.no_e2e and world == 1 and dist is None:
        from ghostm_amd.native import BIN_PATH

        runs, files_ok = [], []
        for _ in range(3):
            if os.path.exists(out_path):
                os.remove(out_path)
            os.sync()
            time.sleep(float(os.environ.get("GHOSTM_BENCH_SETTLE_S", "1.0")))
            te = time.perf_counter()
            rc = subprocess.run([BIN_PATH, "aln"] + argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                timeout=600).returncode
            runs.append(time.perf_counter() - te)
            ok_file = rc == 0 and os.path.exists(out_path) and _sha_file(out_path) == (
                pin["sha256"] if pin else timed_sha)
            files_ok.append(ok_file)
        dt = sorted(runs)[len(runs) // 2]
        e2e_cold = {"seconds": dt, "value": total_res / args.steps / dt, "unit": "query residues/s",
                    "runs_s": runs, "statistic": "median of 3",
                    "includes": "a fresh `ghostm aln` process per run (ghostm_amd/bin/ghostm, GhostmAlignMain): "
                                "process and HIP runtime start, query/DB/index file loads from a warm page "
                                "cache, H2D, the search and the output file written while it runs, process exit",
                    "output_files_match_reference" if pin else "output_files_match_timed_run": all(files_ok)}
        if not all(files_ok):
            matches = False

    k = args.steps
    per = {key: v / k for key, v in st_acc.items()}
    cpu = cpu_all = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu:  # the CPU baseline is an N=1 figure
        n1 = args.cpu_sample or w.get("cpu_sample", 10000)
        nall = args.cpu_sample_all or w.get("cpu_sample_all", 16000)
        cpu = cpu_baseline(workdir, preset, dbprefix, min(n1, nq), aln_args)
        cpu_all = cpu_baseline_all_cores(workdir, preset, dbprefix, min(nall, nq), aln_args)
    ok = matches is not False and all(c is None or c.get("bit_identical_to_gpu_on_sample", True)
                                      for c in (cpu, cpu_all))
    if rank == 0:
        score_t = per["seconds_score"] / max(1, per["score_launches"])
        score_cells = per["score_cells"] / max(1, per["score_launches"])
        achieved = score_cells * SCORE_OPS_PER_CELL / score_t / 1e12 if score_t > 0 else 0.0
        packed = per["score_launches_packed"] == per["score_launches"] and per["score_launches"] > 0
        half = packed and per["score_launches_half"] == per["score_launches"]
        peak = PEAK_VALU_PK16_TOPS if packed else PEAK_VALU_TOPS
        framed = half and per.get("score_launches_framed", 0) == per["score_launches"]
        swar = framed and per.get("score_launches_swar", 0) == per["score_launches"]
        unit = swar and per.get("score_launches_unit", 0) == per["score_launches"]
        n_pair = per.get("score_launches_pair", 0)
        pair = swar and n_pair == per["score_launches"]
        if pair:
            kname = ("k_score_pair<32> (K2 Gotoh DP over a query-independent pair table: one LDS word per "
                     "(query residue, two subject residues), 16-bit integer patterns, two candidates per lane; "
                     "sparse segments)")
        elif swar and n_pair:
            kname = (f"k_score_pair<32> on {n_pair:g} of {per['score_launches']:g} launches per step, "
                     "k_score16f<32,swar> on the rest (K2 Gotoh DP over 16-bit integer patterns)")
        elif unit:
            kname = ("k_score16f<32,swar,unit> (K2 Gotoh DP, per-column frame over 16-bit integer patterns, "
                     "two candidates per lane; unit-pair profile words: the diagonal sum is one op_sel "
                     "v_pk_mad_u16)")
        elif swar:
            kname = ("k_score16f<32,swar> (K2 Gotoh DP, per-column frame over 16-bit integer patterns: packed "
                     "f16 max3 on the patterns, v_add_u32 for the constant adds, two candidates per lane)")
        elif framed:
            kname = ("k_score16f<32> (K2 Gotoh DP, exact integers in packed f16 lanes, per-column frame, "
                     "two candidates per lane)")
        elif half:
            kname = "k_score16<32,f16> (K2 Gotoh DP, exact integers in packed f16 lanes, two candidates per lane)"
        elif packed:
            kname = "k_score16<32,int16> (K2 Gotoh DP, packed int16, two candidates per lane)"
        else:
            kname = "k_score (K2 Gotoh DP, int32)"
        dtype = ("int (exact 16-bit integers; packed f16 max3 orders their patterns, no guard)" if swar
                 else "int (exact integers in packed f16 lanes, int16 re-score above the guard)" if half
                 else "int16" if packed else "int32")
        # the PMC summary of this preset's workload (tools/profile.sh <round> <preset>)
        pmc_path = os.path.join(REPO, "profiles", f"pmc_traffic_{preset}.json")
        if not os.path.exists(pmc_path):
            pmc_path = PMC
        pmc = _json(pmc_path)
        # counters count only for the library being timed: the PMC summary
        # records the profiled library's source hash (tools/pmc_summary.py)
        from ghostm_amd import native, srchash

        timed_hash = srchash.info_hash((native.load().GhostmBuildInfo() or b"").decode())
        pmc_hash = pmc.get("library_src_hash") if pmc else None
        pmc_ok = bool(pmc and pmc.get("queries") == nq and pmc.get("preset", "cfg4") == preset
                      and world == 1 and not args.aln and pmc_hash is not None and pmc_hash == timed_hash)
        pmc_source = {"file": os.path.relpath(pmc_path, REPO) if pmc else None, "round": (pmc or {}).get("round"),
                      "profiled_library_src_hash": pmc_hash, "timed_library_src_hash": timed_hash,
                      "used": pmc_ok}
        issue = _json(VALU_ISSUE)
        roof = {
            "bound": "valu",
            "kernel": kname,
            "achieved": achieved,
            "peak": peak,
            "unit": "Tops/s",
            "frac": achieved / peak,
            "traffic": pmc.get("k_score_hbm_bytes_per_launch") if pmc_ok else None,
            "cells_per_launch": score_cells,
            "ops_per_cell": SCORE_OPS_PER_CELL,
            "gcups": score_cells / score_t / 1e9 if score_t > 0 else 0.0,
            "avg_launch_ms": score_t * 1e3,
            "guard_rescores_per_step": per.get("score_rechecks", 0),
            "launches_per_step": {"pair": n_pair, "unit": per.get("score_launches_unit", 0),
                                  "total": per["score_launches"]},
            # traffic / valu_* come from this PMC summary only when it was recorded
            # on a library with the timed library's source hash (else null)
            "pmc_source": pmc_source,
        }
        if issue and pmc_ok and pmc.get("k_score_valu_insts_per_launch"):
            rate = pmc["k_score_valu_insts_per_launch"] / score_t
            roof["valu_insts_per_launch"] = pmc["k_score_valu_insts_per_launch"]
            roof["issue_rate_ginst_s"] = rate / 1e9
            # the issue ceiling priced by instruction class: K2's column bodies
            # (tools/isa_mix.py, profiles/r3_k2_isa_mix.json) hold n3 VOP3-class
            # and n2 fast-VOP2 instructions; measured costs (tools/microbench,
            # profiles/r2_valu_issue.json): VOP3-class 4.16 shader cycles, fast
            # VOP2 2.27 alone and 3.44 at best inside VOP3P streams (the 1:2 mix
            # row). The ceiling takes the cheapest cost of each class, so the
            # kernel's PMC cycles per instruction cannot beat it.
            mix = (_json(ISA_MIX_PAIR if pair else ISA_MIX_UNIT if unit else ISA_MIX) or {}).get("column_bodies")
            if swar and n_pair and not pair:
                mix = None  # mixed kinds: no single instruction mix
            cyc = pmc.get("k_score_valu_cycles_per_inst")
            c3 = issue.get("cycles_per_inst", {}).get("vop3_class_median")
            if mix and cyc and c3:
                n3, n2 = mix["vop3_class"], mix["fast_vop2"]
                c2_alone = issue["cycles_per_inst"]["fast_vop2_median"]
                ceil_mix = (n3 * c3 + n2 * VOP2_IN_MIX_CYCLES) / (n3 + n2)
                ceil_alone = (n3 * c3 + n2 * c2_alone) / (n3 + n2)
                roof["issue_ceiling"] = {
                    "column_body_vop3_class": n3,
                    "column_body_fast_vop2": n2,
                    "ceiling_cycles_per_inst": ceil_mix,
                    "ceiling_cycles_per_inst_vop2_alone": ceil_alone,
                    "kernel_cycles_per_inst": cyc,
                    "frac": ceil_mix / cyc,
                    "frac_vop2_alone": ceil_alone / cyc,
                    "effective_clock_ghz": pmc.get("k_score_effective_clock_ghz"),
                }
        # K3 per SURVEY §8 d3: TB work = sum over hits of L x the reference's reverse
        # window (L + 2e*2R columns back from the hit's end, clipped at position 0
        # and broken at END; aligner.cpp:775, 806-809, 829-830) at 20 ops per cell.
        # That is exactly the cells k_tb_scan computes (traceback_scan_cells), so
        # the headline is those cells x 20 over the whole K3 time, against the
        # packed 16-bit peak the kernels issue at (both K3 kernels are packed
        # two hits per lane or cheaper). The two kernels are also priced alone:
        # the scan at K2's 10 ops per cell, the key DP's own cells (columns
        # 0..j*, strips 0..i*) at 20 ops against the int32 peak (one hit per lane).
        tb_t = per["seconds_traceback"]
        tb_scan_t = per.get("seconds_traceback_scan", 0.0)
        tb_key_t = max(0.0, tb_t - tb_scan_t)
        scan_cells = per["traceback_scan_cells"]
        key_cells = per["traceback_cells"]
        tb_ach = scan_cells * TB_OPS_PER_CELL / tb_t / 1e12 if tb_t > 0 else 0.0
        scan_ach = scan_cells * SCORE_OPS_PER_CELL / tb_scan_t / 1e12 if tb_scan_t > 0 else 0.0
        key_ach = key_cells * TB_OPS_PER_CELL / tb_key_t / 1e12 if tb_key_t > 0 else 0.0
        roof_k3 = {
            "bound": "valu",
            "kernel": "K3 traceback per step (k_tb_prep/k_tb_pairs/sorts + k_tb_scan scores-only reverse scan "
                      "+ k_traceback_key over columns 0..j*)",
            "definition": "SURVEY §8 d3: sum over hits of L x reverse-window columns (to END / position 0) "
                          "x 20 ops, / K3 device time per step, vs the packed 16-bit VALU peak",
            "achieved": tb_ach,
            "peak": PEAK_VALU_PK16_TOPS,
            "unit": "Tops/s",
            "frac": tb_ach / PEAK_VALU_PK16_TOPS,
            "cells_per_step": scan_cells,
            "ops_per_cell": TB_OPS_PER_CELL,
            "ms_per_step": tb_t * 1e3,
            "scan": {"kernel": "k_tb_scan (+ prep, pairs, the two counting sorts)", "cells_per_step": scan_cells,
                     "ops_per_cell": SCORE_OPS_PER_CELL, "ms_per_step": tb_scan_t * 1e3,
                     "tcups": scan_cells / tb_scan_t / 1e12 if tb_scan_t > 0 else 0.0,
                     "achieved": scan_ach, "peak": PEAK_VALU_PK16_TOPS, "frac": scan_ach / PEAK_VALU_PK16_TOPS},
            "key_dp": {"kernel": "k_traceback_key (columns 0..j*, strips 0..i*)", "cells_per_step": key_cells,
                       "ops_per_cell": TB_OPS_PER_CELL, "ms_per_step": tb_key_t * 1e3,
                       "achieved": key_ach, "peak": PEAK_VALU_TOPS, "frac": key_ach / PEAK_VALU_TOPS},
        }
        seed_gbs = per["seed_bytes"] / per["seconds_seed"] / 1e9 if per["seconds_seed"] > 0 else 0.0
        roof_k1 = {
            "bound": "hbm (nominal; PMC shows the hash kernels issue/latency-bound, see the valu fields)",
            "kernel": "K1 seed stage per step (k_seed_lists, k_seed_hash, k_compact: gathers of CSR positions)",
            "achieved": seed_gbs,
            "peak": PEAK_HBM_GBS,
            "unit": "GB/s",
            "frac": seed_gbs / PEAK_HBM_GBS,
            "algorithmic_bytes_per_step": per["seed_bytes"],
            "traffic": pmc.get("k1_hbm_bytes_per_step") if pmc_ok else None,
            "ms_per_step": per["seconds_seed"] * 1e3,
            "queries_per_class": [per.get(f"seed_queries_class{c}", 0) for c in range(4)],
            "pmc_source": pmc_source,
        }
        if issue and pmc_ok and pmc.get("k1_valu_insts_per_step"):
            rate = pmc["k1_valu_insts_per_step"] / per["seconds_seed"]
            roof_k1["valu_insts_per_step"] = pmc["k1_valu_insts_per_step"]
            roof_k1["issue_rate_ginst_s"] = rate / 1e9
            roof_k1["frac_of_measured_issue"] = rate / 1e9 / issue["packed_vop3_ginst_s"]
            if per.get("seed_list_entries"):
                # wave-instructions per k-mer list entry (a wave-instruction = 64 lane slots)
                roof_k1["valu_insts_per_list_entry"] = pmc["k1_valu_insts_per_step"] / per["seed_list_entries"]
        out = {
            "metric": "query residues aligned/sec (whole node) + bit-identical hit-list vs CPU",
            "value": total_res / elapsed if ok else None,
            "unit": "query residues/s",
            "n_gpus": physical,
            "ranks": world,
            "steps": k,
            "warmup": args.warmup,
            "ms_per_step": elapsed / k * 1e3,
            "step_ms_rank0": step_ms,
            # value: the resident step (the bench contract: inputs already in HBM
            # when the timed region starts). SURVEY §8 d1's wall time of `aln` (file
            # loads, H2D, search, output write) is reported beside it twice:
            # value_end_to_end_warm (sessions back to back in this process) and
            # value_end_to_end_cold (a fresh `ghostm aln` process per run)
            "value_is": "resident step: query/DB/index already in HBM; one step = K1 seed, K2 score, K4 merge, "
                        "K3 traceback, E-values and the whole output text in host memory (N > 1: + the record "
                        "gather); file loads, H2D and the file write are in value_end_to_end_*",
            "value_end_to_end_warm": e2e["value"] if (e2e and ok) else None,
            "value_end_to_end_cold": e2e_cold["value"] if (e2e_cold and ok) else None,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": dtype,
            "data": f"synthetic (ghostm synth; {w['workload']}; aln options "
                    f"{' '.join(os.path.basename(a) for a in aln_args) if aln_args else 'defaults (BLOSUM62 11/1)'})",
            "config": {
                "workload": w["workload"] + ("" if nq == w["queries"] else f" (first {nq} queries)"),
                "aln_options": [os.path.basename(a) for a in aln_args],
                "queries": nq,
                "query_residues_per_step": total_res / k,
                "candidates_per_rank_step": per["candidates"],
                "hits_per_rank_step": per["hits"],
                "segments_per_rank_step": per.get("segments", 0),
                "parallelism": f"query shards x{world} (one process per GPU, balanced, name-group aligned; "
                               "RCCL gather of hit records to rank 0)",
            },
            "full_output_matches_reference": matches if pin else None,
            "output_matches_unsharded_run": gather_check["assembled_file_equals_unsharded"] if gather_check else None,
            "gather_check": gather_check,
            "gather_fill": dict(fills, backend="nccl" if coll_dev == "cuda" else "gloo")
            if gatherer is not None else None,
            "per_rank": per_rank,
            "full_output_reference": (f"sha256 {pin['sha256'][:16]}..., {pin['lines']} lines "
                                      f"(tests/golden/full_golden.json)") if pin else None,
            "roofline": roof,
            "roofline_k1": roof_k1,
            "roofline_k3": roof_k3,
            "stages_s_per_step": {
                "total": per["seconds_total"],
                "seed_device": per["seconds_seed"],
                "score_device": per["seconds_score"],
                "traceback_device": per["seconds_traceback"],
                "merge_select_host_wall": per["seconds_merge"],
                "output_host_background": per["seconds_output"],
            },
            "end_to_end": e2e,
            "end_to_end_cold": e2e_cold,
            "cpu_baseline": cpu,
            "cpu_baseline_all_cores": cpu_all,
        }
        print(json.dumps(out), flush=True)
    sess.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and not args.workdir:
        shutil.rmtree(workdir, ignore_errors=True)
    if rank == 0 and not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
