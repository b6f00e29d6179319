"""Benchmark of the block-Hungarian round (BASELINE.json metric).

One step = one full round of the reference's loop on synthetic Kaggle-shaped
data (1M children, 1000 gift types x 1000 units, seed 2017): sample every
disjoint block of the round (3730 singles blocks at n=256; 78 twin blocks at
256 pairs), build + solve + apply them on the GPU(s), re-synchronise the gift
vector across ranks (RCCL all-gather, N > 1) and re-score the whole
assignment (avg_normalized_happiness), reading the score back as the
reference does every round (mpi_single.py:157-169).

`--gpus N` (N > 1) without a torch.distributed environment starts N ranks
itself (`torch.distributed.run`, a child process; this process touches no
GPU) and forwards rank 0's line.  Prints ONE JSON line (rank 0).  value =
blocks solved and applied per second, whole job; score gain per second is
reported beside it.

A plain run sets up, warms up, times `--steps` rounds and prints the line
(`ms_per_step` = wall time of one timed round).  `--full` adds what the
headline does not need: the CPU baselines (B1, the C port, scipy; timed before
the GPU run) and the roofline's latency / LDS view (lone-block launches after
it).  `--dump-outputs DIR` writes what the timed rounds returned (dump_outputs).
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "mpi-hungarian-method_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
# LDS: 256 CUs x 256 B/clk (ds_read_b64/b128 rate per CU, MI355X_MICROARCH.md
# LDS table) x 2.4 GHz
LDS_PEAK_TBS = 256 * 256 * 2.4e9 / 1e12
# Algorithmic LDS bytes of the solve per Dijkstra step and per Dijkstra (all
# lanes of the block's waves): santa_sp3_kernel per step =
# 64 lanes x (4 scatter + 16 row read + 4 un-scatter + 4 u + 1 + 1 remaining),
# per Dijkstra 64 x (4 remaining + 16 dual atomics); santa_dt_kernel per step = 64 lanes x 4
# tile bytes + 16 (u, mover, two one-lane stores), per Dijkstra 64 x (16 remaining + 16 dual
# atomics + 4 path rows); the 4-wave kernels per step = 256 threads
# x (1 tile byte + 4 u + 8 step word) + the fold, per Dijkstra 256 x 12.
LDS_BYTES = {"santa_sp3_kernel": (64 * 30, 64 * 20), "santa_dt_kernel": (64 * 4 + 16, 64 * 36),
             "santa_block_kernel": (256 * 13, 256 * 12), "santa_vt_kernel": (256 * 12, 256 * 12)}
CLOCK_HZ = 2.4e9               # MI355X max shader clock (MI355X_MICROARCH.md)
KERNEL_SRC = os.path.join(ROOT, "mpi-hungarian-method_amd", "csrc", "santa_hip.hip")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["single", "twins", "triplets"], default="single",
                    help="triplets: the 3-slot unit extension (not a reference script)")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--seed", type=int, default=2017)
    ap.add_argument("--cpu-seconds", type=float, default=12.0,
                    help="budget of the CPU port / scipy baselines (rank 0, before the GPU run)")
    ap.add_argument("--b1-seconds", type=float, default=6.0,
                    help="budget per rank count of the reference-semantics baseline B1")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: leave the CPU baselines out")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure: the CPU baselines (B1, the C port, scipy) before "
                         "the GPU run and the latency / LDS view of the roofline (lone-block launches "
                         "after it); a plain run only sets up, warms up, times the steps and prints")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the round loop returned for them as "
                         "DIR/<name>.npy (rank 0): the assignment and every timed round's sums and score")
    ap.add_argument("--score-check-every", type=int, default=None,
                    help="0: rescore the whole state every round (the reference); K: the round's sums "
                         "from the block kernels' exact deltas (all-reduced at N > 1) with a full "
                         "rescore every K rounds that must agree (default 16, every N)")
    ap.add_argument("--dist-backend", default="nccl",
                    help="test only: 'gloo' with --one-device rehearses N ranks on one GPU")
    ap.add_argument("--one-device", action="store_true",
                    help="test only: every rank uses cuda:0 (functional N>1 runs on a 1-GPU box)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        args.no_cpu_baseline = True
    return args


# --------------------------------------------------------------------------- launcher
def launch_ranks(args) -> int:
    """`bench.py --gpus N` run by hand: start the N ranks as a child
    `torch.distributed.run` (one process per GPU, rendezvous on 127.0.0.1;
    the reference's `mpirun -np P`) and exit with its code.  Rank 0's JSON
    line reaches stdout through the inherited descriptors."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # the CPU baselines run here, before any rank exists (this process touches
    # no GPU), and reach rank 0 through a file
    path = None
    if not args.no_cpu_baseline and CPU_JSON_ENV not in env:
        import tempfile
        cb = cpu_baselines(args, cpu_info())
        fd, path = tempfile.mkstemp(prefix="santa_bench_cpu_", suffix=".json")
        with os.fdopen(fd, "w") as f:
            json.dump(cb, f)
        env[CPU_JSON_ENV] = path
    env.setdefault("OMP_NUM_THREADS", "1")
    try:
        return subprocess.call(cmd, env=env)
    finally:
        if path:
            os.unlink(path)


# --------------------------------------------------------------------------- CPU side
def cpu_info() -> dict:
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    omp = os.environ.get("OMP_NUM_THREADS")
    aff = len(os.sched_getaffinity(0))
    # the GPU box leases a CPU share per GPU and says so in OMP_NUM_THREADS
    # (os.cpu_count() there shows the whole machine); otherwise the affinity
    used = int(omp) if omp and omp.isdigit() and int(omp) > 0 else aff
    return {"model": model, "nproc": os.cpu_count(), "affinity": aff, "omp_num_threads": omp,
            "used": min(used, aff)}


def b1_baseline(mode: str, n: int, cores: int, seconds: float, max_procs: int | None = None) -> dict:
    """B1: the reference's own round loop as written —
    P ranks, Python n^2 cost loop, scipy, pickled gather/bcast, full rescore
    and the 1M-row CSV every round (oracle/ref_semantics.py) — at P = 8 and
    P = all leased cores, at most `max_procs` (the blocks of a round: with
    more ranks than twin blocks the reference raises IndexError,
    mpi_twins.py:128,132).  Runs as a child process before this process
    touches the GPU."""
    cap = min(cores, max_procs) if max_procs else cores
    procs = sorted({min(8, cap), cap})
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "ref_semantics.py"), "--mode", mode,
           "--n", str(n), "--procs", ",".join(map(str, procs)), "--seconds", str(seconds)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60 + 4 * seconds * len(procs))
        out = json.loads(r.stdout.strip().splitlines()[-1])
    except (subprocess.SubprocessError, ValueError, IndexError) as e:
        return {"error": f"{type(e).__name__}: {e}"}
    return {"blocks_per_s": {str(x["procs"]): x["blocks_per_s"] for x in out["runs"]},
            "score_gain_per_s": {str(x["procs"]): x["score_gain_per_s"] for x in out["runs"]},
            "rounds": {str(x["procs"]): x["rounds"] for x in out["runs"]},
            "setup_s": out["setup_s"]}


CPU_JSON_ENV = "SANTA_BENCH_CPU_JSON"


def cpu_baselines(args, cpu: dict) -> dict:
    """Every CPU figure of the line, timed before this process touches the GPU
    (rank 0, or the `--gpus N` launcher before it starts the ranks): B1 (the
    reference's round as written, in a child process), the C port of the path
    on the leased cores and saturated scipy.  Same workload as the GPU line."""
    from santa_hip import data as D
    from santa_hip.sampler import family_sizes, twin_geometry
    sd = D.synthetic(args.seed)
    mode = {"single": 0, "twins": 1, "triplets": 2}[args.mode]
    # (B1 runs on its own synthetic instance of the same shape: same twin count)
    cap = twin_geometry(*family_sizes(sd.nc), args.n)[2] if mode == 1 else None
    b1 = b1_baseline(args.mode, args.n, cpu["used"], args.b1_seconds, cap) if args.mode != "triplets" else None
    cb = cpu_baseline(sd, mode, args.n, args.cpu_seconds, cpu["used"])
    cb["cpu_model"] = cpu["model"]
    cb["nproc"] = cpu["nproc"]
    if b1 is not None and "blocks_per_s" in b1:
        cb["b1_blocks_per_s"] = b1["blocks_per_s"]
        cb["b1_score_gain_per_s"] = b1["score_gain_per_s"]
        script = "mpi_single.py:119-181" if args.mode == "single" else "mpi_twins.py:121-187"
        cb["b1_sample"] = (f"oracle/ref_semantics.py: the reference's round as written "
                           f"({script}) with P ranks = {list(b1['blocks_per_s'])} "
                           f"worker processes, {b1['rounds']} rounds in {args.b1_seconds}s each: "
                           f"P blocks per round, Python n^2 cost loop, scipy, pickled "
                           f"gather/bcast, full rescore and the 1M-row CSV per round")
    elif b1 is not None:
        cb["b1_error"] = b1.get("error")
    cb["timed"] = "before the GPU run, on the host cores this rank (or the launcher) leases"
    cb["whole_node"] = whole_node_cpu(cb, cpu)
    return cb


def whole_node_cpu(cb: dict, cpu: dict) -> dict:
    """The CPU comparator of the whole host (every thread the machine has:
    the reference's `mpirun -np <all cores>` on the node of an 8-GPU line),
    projected from the figures measured on the leased cores: per-thread rate
    x host threads.  The GPU box leases `used` of the host's threads and its
    pool rules size worker pools to that share, so the whole node is not
    timed; blocks of a round are independent (no communication inside a
    solve), so linear scaling is an upper bound for the CPU -- it flatters
    the CPU, never the GPU.  A round's blocks are its only parallelism (each
    waits for the previous round's state): with fewer blocks than threads
    (78 twins blocks, 6 at 3000 pairs) at most `round_blocks` threads work, so
    both the measured and the projected thread counts are capped there."""
    used = max(int(cb.get("cores") or cpu.get("used") or 1), 1)
    node = max(int(cpu.get("nproc") or used), used)
    nb = int(cb.get("round_blocks") or node)
    busy, node_busy = min(used, nb), min(node, nb)
    per = node_busy / busy
    out = {"kind": "projected", "cores": node_busy, "from_cores": busy, "factor": round(per, 3),
           "round_blocks": nb,
           "port_blocks_per_s": round(cb.get("value", 0.0) * per, 1),
           "reference_lap_blocks_per_s": round(cb.get("reference_lap_blocks_per_s", 0.0) * per, 1),
           "note": f"measured on {used} leased threads ({busy} busy) x {node_busy}/{busy}: linear "
                   f"scaling of independent blocks over min(host threads {node}, blocks per round "
                   f"{nb}), an upper bound for the CPU"}
    b1 = cb.get("b1_blocks_per_s") or {}
    if b1:
        p = max(b1, key=int)  # the largest P measured
        out["b1_blocks_per_s"] = round(b1[p] * node_busy / int(p), 2)
        out["b1_from_procs"] = int(p)
    return out


def cpu_baseline(sd, mode: int, n: int, seconds: float, cores: int):
    """The oracle (plain-C port of the reference path: cost build + scipy-exact
    SAP + apply) on the host cores over blocks of the same round: one thread
    per core (ctypes releases the GIL; blocks are disjoint, so the threads
    share the type vector safely), and a single-core figure beside it."""
    import concurrent.futures as cf
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from santa_hip.sampler import sample_blocks, single_geometry, triplet_geometry, twin_geometry
    tri, tw = sd.families
    if mode == 0:
        lo, count, nb = single_geometry(sd.nc, n, tri, tw)
        stride = 1
    elif mode == 2:
        lo, count, nb = triplet_geometry(tri, n)
        stride = 3
    else:
        lo, count, nb = twin_geometry(tri, tw, n)
        stride = 2
    rows = sample_blocks(12345, 0, lo, count, stride, n, nb)
    t = sd.types.copy()
    done1 = 0
    t0 = time.perf_counter()
    while done1 < nb and time.perf_counter() - t0 < seconds / 4:
        oracle.round_blocks(mode, sd.wish, t, rows[done1:done1 + 8], ng=sd.ng)
        done1 += min(8, nb - done1)
    el1 = time.perf_counter() - t0
    t = sd.types.copy()
    deadline = time.perf_counter() + seconds
    doneN = 0

    def work(ch):
        if time.perf_counter() > deadline:
            return 0
        oracle.round_blocks(mode, sd.wish, t, ch, ng=sd.ng)
        return len(ch)

    t1 = time.perf_counter()
    with cf.ThreadPoolExecutor(cores) as ex:
        rnd = 0
        while time.perf_counter() < deadline:
            rr = rows if rnd == 0 else sample_blocks(12345, rnd, lo, count, stride, n, nb)
            for k in ex.map(work, [rr[i:i + 4] for i in range(0, nb, 4)]):
                doneN += k
            rnd += 1
    elN = time.perf_counter() - t1
    t2 = time.perf_counter()
    oracle.score_sums(sd.wish, sd.goodkids, t)  # the full rescore of each round, 1 core
    score_s = time.perf_counter() - t2
    bpsN = doneN / elN if elN > 0 else 0.0
    sc_bps, sc_done, sc_el = scipy_baseline(sd, mode, n, min(6.0, seconds / 2), cores, rows, lo, count,
                                            stride, nb)
    return {"value": round(bpsN, 2), "unit": "blocks/s", "cores": cores, "kind": "port",
            "round_blocks": nb,
            "sample": f"{doneN} blocks (n={n}, rounds of {nb}) through oracle.round_blocks "
                      f"on {cores} threads in {elN:.1f}s; {done1} blocks on 1 core in {el1:.1f}s; "
                      f"full rescore {score_s:.2f}s per round (1 core)",
            "single_core_blocks_per_s": round(done1 / el1, 2) if el1 > 0 else None,
            "round_blocks_per_s_incl_score": round(nb / (nb / bpsN + score_s), 2) if bpsN > 0 else None,
            "reference_lap_blocks_per_s": round(sc_bps, 2),
            "reference_lap_sample": f"{sc_done} blocks: the reference's float32 happiness values "
                                    f"(mpi_single.py:213-218) gathered per block with numpy + scipy "
                                    f"linear_sum_assignment (mpi_single.py:101) on {cores} threads "
                                    f"in {sc_el:.1f}s"}


def scipy_baseline(sd, mode, n, seconds, ncores, rows, lo, count, stride, nb):
    """Saturated-scipy comparator: the reference's own LAP
    (scipy, which releases the GIL) on a vectorised build of the reference's
    cost matrix, one thread per core, blocks of successive rounds applied to
    the type vector.  Singles: C[i, j] = child_happiness[child_i][type_j];
    twins: float32 sum of both twins' values (mpi_twins.py:97-103)."""
    import concurrent.futures as cf
    from scipy.optimize import linear_sum_assignment
    from santa_hip.sampler import sample_blocks
    miss = np.float32(1.0 / (2 * sd.n_wish))
    vals = (-2.0 * (sd.n_wish - np.arange(sd.n_wish))).astype(np.float32)
    types = sd.types.copy()

    def table(ch):
        T = np.full((ch.shape[0], sd.ng), miss, dtype=np.float32)
        T[np.arange(ch.shape[0])[:, None], sd.wish[ch]] = vals
        return T

    def one(block):
        if time.perf_counter() > deadline:
            return 0
        t = types[block]
        T = table(block)
        for m in range(1, mode + 1):  # float32, left to right (mpi_twins.py:101)
            T = T + table(block + m)
        _, col = linear_sum_assignment(T[:, t].astype(np.float64))
        for m in range(mode + 1):
            types[block + m] = t[col]
        return 1

    deadline = time.perf_counter() + seconds
    done = 0
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(ncores) as ex:
        rnd = 0
        while time.perf_counter() < deadline:
            rr = rows if rnd == 0 else sample_blocks(54321, rnd, lo, count, stride, n, nb)
            done += sum(ex.map(one, list(rr)))
            rnd += 1
    el = time.perf_counter() - t0
    return (done / el if el > 0 else 0.0), done, el


# --------------------------------------------------------------------------- HBM traffic
def design_kernels(kname: str):
    """The kernels one solve launch of a design may run: the register-tile
    sparse design builds its tiles in santa_sp3_kernel itself (packed
    wishlists, round 4) or in santa_tile_kernel first (other wishlist shapes);
    the events around the solve bracket both.  stored_traffic sums the ones
    the profile saw."""
    k = kname.split(" ")[0].split("<")[0]
    return ["santa_tile_kernel", k] if k == "santa_sp3_kernel" else [k]


def _same_launch(s, blocks, n=256, mode=0):
    """A summary describes this launch only if its probe ran the same number
    of blocks per launch of the same block size and mode (one kernel name
    covers several workloads: the 4-wave santa_block_kernel runs the twins
    round and the 8-GPU singles shard; santa_big_kernel every n > 256).
    (Summaries from before round 4 recorded no n / mode: n = 256, and the
    mode is implied by the block count.)"""
    p = s.get("probe", {})
    return p.get("blocks") == blocks and p.get("n", 256) == n and p.get("mode", mode) == mode


def stored_occupancy(kname: str, blocks: int, n: int = 256, mode: int = 0):
    """Mean resident waves per SIMD and LDS-array activity of `kname` from
    the newest committed PMC summary of THIS kernel source and launch size
    (the "occ" pass of tools/profile_round.sh, round-0 launch), or None."""
    src = hashlib.sha256(open(KERNEL_SRC, "rb").read()).hexdigest()[:16]
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_summary.json")), reverse=True):
        try:
            s = json.load(open(path))
        except (OSError, ValueError):
            continue
        if s.get("source_sha16") == src and _same_launch(s, blocks, n, mode) and kname in s.get("occupancy_lds", {}):
            e = dict(s["occupancy_lds"][kname])
            e["source"] = f"{os.path.basename(path)} (round-0 launch, kernel source {src})"
            return e
    return None


def stored_traffic(knames, blocks: int, n: int = 256, mode: int = 0):
    """HBM bytes per launch of the kernels `knames` (summed) from the newest committed rocprofv3 PMC
    summary taken on THIS kernel source (tools/profile_round.sh ->
    profiles/<tag>_summary.json records the source hash).  Each kernel's
    FETCH_SIZE is scaled by the factor calibrated for its access pattern
    (tools/calib/gather_calib.hip, profiles/<tag>_fetch_calibration.json:
    kernel_factors -- the tile build's one-line packed rows, the solve's
    16 B/lane record stream -- else the 8-byte row-gather factor); WRITE_SIZE
    is taken as read."""
    src = hashlib.sha256(open(KERNEL_SRC, "rb").read()).hexdigest()[:16]
    calib = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_fetch_calibration.json")))
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_summary.json")), reverse=True):
        try:
            s = json.load(open(path))
        except (OSError, ValueError):
            continue
        if s.get("source_sha16") != src or not _same_launch(s, blocks, n, mode):
            continue
        hb = s.get("hbm_bytes_per_launch", {})
        # the kernels this summary saw the launch run (the last named is the
        # design's main kernel, always required); filtered per summary, so a
        # summary without the optional build kernel does not drop it from the next
        names = [k for k in knames[:-1] if k in hb] + knames[-1:]
        es = [hb.get(k, {}) for k in names]
        if all("FETCH_SIZE_bytes" in e and "WRITE_SIZE_bytes" in e for e in es):
            cal = json.load(open(calib[-1])) if calib else {}
            ks = [cal.get("kernel_factors", {}).get(kn, cal.get("gather_correction_factor", 1.0)) for kn in names]
            fetch = sum(e["FETCH_SIZE_bytes"] for e in es)
            write = sum(e["WRITE_SIZE_bytes"] for e in es)
            est = sum(e["FETCH_SIZE_bytes"] * k for e, k in zip(es, ks)) + write
            return {"traffic": round(est),
                    "traffic_raw": {"FETCH_SIZE": fetch, "WRITE_SIZE": write, "kernels": names,
                                    "fetch_correction": ks,
                                    "calibration": os.path.basename(calib[-1]) if calib else None},
                    "traffic_source": f"{os.path.basename(path)} (kernel source {src})"}
    return {"traffic": None,
            "traffic_note": f"no committed PMC summary was taken on this kernel source ({src}) "
                            f"at {blocks} blocks of n = {n} per launch"}


# --------------------------------------------------------------------------- outputs
def dump_outputs(path: str, types, res) -> None:
    """What a caller of the timed round loop holds after its last round, one
    .npy per array: the gift type of every child (`types`, updated in place;
    type ids are below 2^24, exact in float32) and the loop's result, i.e. the
    exact integer (S_child, S_gift) and the score of every timed round and the
    best score (float64; the sums stay far below 2^53).  About 4 MB at 1M
    children.  The data, the block samples and the solver are seeded and
    integer-exact, so two runs with the same arguments write the same bytes."""
    os.makedirs(path, exist_ok=True)
    h = res.history
    np.save(os.path.join(path, "types.npy"), types.cpu().numpy().astype(np.float32))
    np.save(os.path.join(path, "round_sums.npy"),
            np.array([[st.s_child, st.s_gift] for st in h], dtype=np.float64).reshape(len(h), 2))
    np.save(os.path.join(path, "round_scores.npy"), np.array([st.score for st in h], dtype=np.float64))
    np.save(os.path.join(path, "best_score.npy"), np.array([res.best_score], dtype=np.float64))


# --------------------------------------------------------------------------- main
def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with "
                 f"--nproc-per-node {args.gpus} or drop WORLD_SIZE")
    local = 0 if args.one_device else int(os.environ.get("LOCAL_RANK", "0"))
    cpu = cpu_info()
    # the CPU baselines first, while nothing here has touched the GPU (rank 0
    # only; the other ranks wait in the rendezvous), or the launcher's
    # (the reference has no triplet script: no B1 for the triplet extension)
    cpu_line = None
    if rank == 0 and not args.no_cpu_baseline:
        pre = os.environ.get(CPU_JSON_ENV)
        if pre and os.path.exists(pre):
            with open(pre) as f:
                cpu_line = json.load(f)
        else:
            cpu_line = cpu_baselines(args, cpu)

    import torch
    import santa_hip
    from santa_hip import _lib
    from santa_hip import data as D
    from santa_hip.context import SantaGPU
    from santa_hip.driver import GPUEngine, World, run_rounds, shard_range

    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import datetime

        import torch.distributed as dist
        wait = datetime.timedelta(minutes=30)  # (rank 0 may time the CPU baselines first)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=wait)  # RCCL over xGMI
        else:
            dist.init_process_group(args.dist_backend, timeout=wait)
    mode = {"single": _lib.SH_MODE_SINGLE, "twins": _lib.SH_MODE_TWINS,
            "triplets": _lib.SH_MODE_TRIPLETS}[args.mode]
    n = args.n
    sd = D.synthetic(args.seed)
    ctx = SantaGPU.from_data(sd, local)
    types = ctx.upload_types(sd.types)
    _, _, _, nb = ctx.geometry(mode, n)
    b0, b1_, _ = shard_range(nb, rank, world)
    my_blocks = b1_ - b0
    w = World(rank, world, None)
    stream = torch.cuda.current_stream(dev)
    max_calls = 2 * max(args.steps, 1) + 2  # (keep-if-improved rounds may be re-run)
    steps_dev = torch.zeros((max_calls, max(my_blocks, 1)), dtype=torch.int64, device=dev)

    class BenchEngine(GPUEngine):
        """GPUEngine with HIP events (on the launch stream) and the Dijkstra
        step counts of every timed solve launch."""

        def __init__(self, c):
            super().__init__(c)
            self.timed = False
            self.ev = []

        # every timed launch counts its Dijkstra steps; every EV_EVERY-th one
        # from the EV_OFFSET-th on is also bracketed by the events: an event
        # record is a marker packet on the stream, ~5 us of idle GPU between
        # two rounds' kernels (profiles/r05l_round_gaps.json against r05m's
        # un-instrumented loop).  Rounds 1, 5, 9, ...: round 0, twice as long
        # as the rest, biased a sample that held it (the kernel average then
        # came out above the round time)
        EV_EVERY = 4
        EV_OFFSET = 1

        def solve_blocks(self, mode_, rows_, n_, types_, delta=None, steps=None):
            if not self.timed:
                return super().solve_blocks(mode_, rows_, n_, types_, delta=delta)
            k = self.calls
            self.calls += 1
            st = steps_dev[k] if k < max_calls else None
            if k % self.EV_EVERY != self.EV_OFFSET:
                return super().solve_blocks(mode_, rows_, n_, types_, delta=delta, steps=st)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            super().solve_blocks(mode_, rows_, n_, types_, delta=delta, steps=st)
            e1.record(stream)
            self.ev.append((e0, e1, k))

    eng = BenchEngine(ctx)
    eng.calls = 0
    eng.EV_OFFSET = BenchEngine.EV_OFFSET if args.steps > 1 else 0
    sc0, sg0, _, _ = ctx.score_sums(types)
    score0 = santa_hip.score_from_sums(sc0, sg0, ctx.nc, ctx.ng, ctx.n_wish, ctx.n_good)

    def rounds(k: int):
        # the reference's round loop (santa_hip.driver.run_rounds), pipelined:
        # round r's score runs on a side stream from a snapshot while round r+1
        # is solved (singles keep every round; twins/triplets keep only
        # improving rounds, speculated and re-run after a rejection); a fixed
        # number of rounds (no patience stop) so every run times K rounds
        return run_rounds(eng, types, mode=mode, n=n, seed=args.seed, max_rounds=k, patience=1 << 30,
                          world=w, score0=score0, sums0=(sc0, sg0), pipeline=True,
                          score_check_every=args.score_check_every)

    # warm up on the same rounds, then restart from the baseline assignment so
    # the timed rounds are rounds 0..K-1 of the optimisation (as in the
    # reference, which starts from baseline_res.csv)
    if args.warmup:
        rounds(args.warmup)
    torch.cuda.synchronize()
    types.copy_(ctx.upload_types(sd.types))
    score_start = score0
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    eng.timed = True
    eng.calls = 0
    t0 = time.perf_counter()
    res = rounds(args.steps)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    eng.timed = False
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, types, res)
    ev = eng.ev
    state = {"best": res.best_score}
    launches = len(ev)
    kern_ms = [a.elapsed_time(b) for a, b, _ in ev] or [0.0]
    kern_avg_s = float(np.mean(kern_ms)) / 1e3
    blocks_total = nb * args.steps
    value = blocks_total / elapsed
    gain = (state["best"] - score_start) / elapsed

    # -- roofline of the dominant kernel (fused cost build + SAP + apply) ------
    design = ctx.solve_design(mode, n, max(my_blocks, 1))
    kname = _lib.SH_DESIGN_NAMES[design]
    per_block = (200 * (mode + 1) + 8) * n  # algorithmic HBM bytes / block
    achieved = per_block * my_blocks / kern_avg_s / 1e9 if kern_avg_s > 0 else 0.0
    # latency / occupancy view from the Dijkstra steps of the TIMED launches:
    # the kernel is a serial chain of Dijkstra steps per block.  The lone
    # per-step latency is measured by re-running round 0's longest block
    # alone (same kernel design, untimed region): launches of their own, --full only.
    latency = None
    lds = None
    if args.full and my_blocks:
        st_all = steps_dev[:min(eng.calls, max_calls), :my_blocks].cpu().numpy().astype(np.int64)
        st = st_all[[k for _, _, k in ev if k < len(st_all)]]  # (the launches the events timed)
        bmax = int(st_all[0].argmax())
        rows0 = ctx.sample_blocks(mode, n, nb, args.seed, 0)
        one = rows0[(b0 + bmax) * n:(b0 + bmax + 1) * n].contiguous()
        force = {0: _lib.SH_FLAG_SP_TILE, 7: _lib.SH_FLAG_SP_TILE, 1: _lib.SH_FLAG_LDS_TILE,
                 8: _lib.SH_FLAG_DT_TILE}.get(design, 0)
        lone = []
        for _ in range(3):
            tt = ctx.upload_types(sd.types)
            s1 = torch.zeros(1, dtype=torch.int64, device=dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx.solve_blocks(mode, one, n, tt, steps=s1, flags=force)
            b.record(stream)
            torch.cuda.synchronize()
            lone.append(a.elapsed_time(b) / 1e3)
        lone_steps = int(s1.item())
        s_per_step = min(lone) / max(lone_steps, 1)
        resident = ctx.resident_blocks(mode, n, my_blocks)
        chain_floor = float(st.max(axis=1).sum()) * s_per_step          # longest block per launch
        occ_floor = float(st.sum()) * s_per_step / max(min(resident, my_blocks), 1)
        kern_sum = float(np.sum(kern_ms)) / 1e3
        floor = max(chain_floor, occ_floor)
        kshort = kname.split(" ")[0]
        lds = None
        if kshort in LDS_BYTES:
            per_step, per_dij = LDS_BYTES[kshort]
            lds_b = float(st.sum()) * per_step + my_blocks * n * per_dij * len(st)
            ach = lds_b / kern_sum / 1e12 if kern_sum > 0 else 0.0
            lds = {"bound": "lds", "achieved": round(ach, 3), "peak": round(LDS_PEAK_TBS, 1), "unit": "TB/s",
                   "frac": round(ach / LDS_PEAK_TBS, 4), "bytes_per_step": per_step, "bytes_per_dijkstra": per_dij,
                   "note": "algorithmic LDS bytes of the solve (steps of the timed launches) / kernel time"}
            occ = stored_occupancy(kshort, my_blocks, n, mode)
            if occ:
                lds["pmc"] = occ
        latency = {"steps_per_launch": float(st.sum(axis=1).mean()),
                   "steps_max_block_per_launch": float(st.max(axis=1).mean()),
                   "round0_steps": int(st_all[0].sum()), "round0_max_block_steps": int(st_all[0].max()),
                   "lone_block_steps": lone_steps, "lone_block_ms": round(min(lone) * 1e3, 4),
                   "cycles_per_step_lone": round(s_per_step * CLOCK_HZ, 1),
                   "resident_blocks": resident,
                   "launches": launches,
                   "chain_floor_ms_per_launch": round(chain_floor / max(len(st), 1) * 1e3, 4),
                   "occupancy_floor_ms_per_launch": round(occ_floor / max(len(st), 1) * 1e3, 4),
                   "binding": "longest block's Dijkstra chain" if chain_floor >= occ_floor else
                              "resident blocks x per-step latency",
                   "frac": round(floor / kern_sum, 4) if kern_sum > 0 else None,
                   "note": "floors are lower bounds on the launch time from the lone per-step latency "
                           "(no co-resident wave contention); frac = floor / measured kernel time"}
    out = {
        "metric": "assignment blocks solved/sec (n=256) + score gain/sec at 1/2/4/8 GPUs",
        "value": round(value, 2),
        "unit": "blocks/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic (seeded Kaggle-shaped: 1M children x 100 wishes, 1000 gifts x 1000 good kids)",
        "config": {"workload": (f"singles full round: {nb} disjoint n={n} blocks/round"
                                + (" (BASELINE config 2)" if n == 256 else " (reference block size)"
                                   if n == 2000 else "")
                                if mode == 0 else
                                f"triplets full round: {nb} disjoint {n}-unit blocks/round (extension)"
                                if mode == 2 else
                                f"twins full round: {nb} disjoint {n}-pair blocks/round"
                                + (" (BASELINE config 3)" if n == 256 else " (reference block size)"
                                   if n == 3000 else "")),
                   "block_n": n, "blocks_per_round": nb,
                   "parallelism": f"blocks sharded over {world} rank(s)"
                                  + (" on one device (test)" if args.one_device and world > 1 else
                                     " = GPU(s)")},
        "score_gain_per_s": gain,
        "score_start": score_start,
        "score_end": state["best"],
        "roofline": {"bound": "latency", "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "hbm_note": "achieved/peak/frac/traffic are the HBM view (algorithmic bytes "
                                 "per block / kernel time); the kernel is bound by its serial "
                                 "Dijkstra chains, see latency",
                     "kernel": kname, "kernel_avg_ms": round(kern_avg_s * 1e3, 4),
                     "kernel_avg_over": f"HIP events around every {eng.EV_EVERY}th timed launch from the "
                                        f"{eng.EV_OFFSET}th ({launches} of {eng.calls}); the floors and LDS "
                                        "bytes over the same launches",
                     "kernel_avg_rounds": [k for _, _, k in ev],
                     "algorithmic_bytes_per_block": per_block, "latency": latency, "lds": lds},
        "cpu": cpu,
    }
    # PMC summaries of the same kernel source and launch size: the full one-GPU
    # round (tools/profile_round.sh) or rank 0's shard at N = 2, 4, 8
    # (tools/profile_shards.sh); else a traffic_note says none was taken
    out["roofline"].update(stored_traffic(design_kernels(kname), my_blocks, n, mode))
    if cpu_line is not None:
        out["cpu_baseline"] = cpu_line
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
