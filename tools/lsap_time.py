"""dev: time the batched LSAP for a few cases on the library SANTA_HIP_LIB selects (A/B).
    python tools/lsap_time.py [--dtype hash|i64|f64|f32|f16|bf16] [--flags N] [--ties] [--duals] [--tag TEXT]
                              [--large] [--oracle]
                              [NxB | NRxNCxB ...]     (default: 256x512 512x256 1024x256 256x4096)
NxB: B square n x n instances; NRxNCxB: B instances of nr x nc.
--dtype hash (the default): lsap_solve_batched_hash / _rect_hash, costs generated in the kernel.
--dtype f64 / f32 / f16 / bf16: solve_batched on a device tensor of that dtype, generated on the
  device from seed 7: torch.rand * 2^16, or with --ties the tie-heavy randint(0, 3) * 0.5.
--dtype i64: solve_batched on an int64 device tensor, randint(0, 2^16) from seed 7.
--duals: solve_batched(duals=True), the lsap_solve_batched_duals_ entries (not with hash).
--large: solve_batched_large, the lsap_solve_large_ entries (up to 4096 rows or columns; not with hash).
--oracle: also time the CPU oracle (scipy's algorithm, one core) on instance 0 of the tensor, once:
  oracle_ms is one instance, to be multiplied by B for the batch.
--flags: C-ABI flags passed on (SH_FLAG_F64_MW = 16384, SH_FLAG_F64_SW = 32768).
Both take comma-separated lists (every combination is timed, per case).  SANTA_HIP_PKG names the
directory that holds the santa_hip package of another checkout (an older commit, with
SANTA_HIP_LIB its own library); the default is this tree's.
One JSON line per case: best and median of 3 timed solves after a warm-up (HIP events, ms)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SANTA_HIP_PKG") or os.path.join(ROOT, "mpi-hungarian-method_amd"))
import torch  # noqa: E402
import santa_hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="hash")
ap.add_argument("--flags", default="0")
ap.add_argument("--ties", action="store_true")
ap.add_argument("--duals", action="store_true")
ap.add_argument("--tag", default=None)
ap.add_argument("--large", action="store_true")
ap.add_argument("--oracle", action="store_true")
ap.add_argument("cases", nargs="*", default=["256x512", "512x256", "1024x256", "256x4096"])
args = ap.parse_args()
DT = {"i64": torch.int64, "f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
dtypes, flag_list = args.dtype.split(","), [int(f) for f in args.flags.split(",")]
assert all(d == "hash" or d in DT for d in dtypes), "--dtype: hash, i64, f64, f32, f16 or bf16"
assert not ((args.duals or args.large or args.oracle) and "hash" in dtypes), \
    "--duals, --large and --oracle need a cost tensor"
solve_batched = santa_hip.solve_batched_large if args.large else santa_hip.solve_batched

for case, dtype, flags in [(tuple(int(x) for x in c.split("x")), d, f)
                           for c in args.cases for d in dtypes for f in flag_list]:
    nr, (n, B) = (case[0], case[1:]) if len(case) == 3 else (None, case)
    if dtype == "hash":
        def solve():
            if nr is None:
                santa_hip.solve_hash(7, 1 << 16, n, B)
            else:
                santa_hip.solve_hash(7, 1 << 16, n, B, nr=nr)
    else:
        g = torch.Generator(device="cuda").manual_seed(7)
        shape = (B, n if nr is None else nr, n)
        if dtype == "i64":
            C = torch.randint(0, 3 if args.ties else 65536, shape, generator=g, device="cuda")
        elif args.ties:
            C = torch.randint(0, 3, shape, generator=g, device="cuda").to(DT[dtype]) * 0.5
        else:
            C = (torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * 65536.0).to(DT[dtype])

        def solve():
            if args.duals:
                solve_batched(C, with_cost=False, flags=flags, duals=True)
            else:
                solve_batched(C, with_cost=False, flags=flags)

    solve()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    out = {"n": n, "B": B, "ms": min(ts)}
    if nr is not None:
        out = {"nr": nr, "nc": n, "B": B, "ms": min(ts)}
    if dtype != "hash" or flags or args.tag:
        out.update(dtype=dtype, flags=flags, ties=args.ties, median_ms=statistics.median(ts))
    if args.duals:
        out["duals"] = True
    if args.large:
        out["large"] = True
    if args.oracle:
        import time
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        C0 = C[0].cpu().numpy()
        C0 = C0 if dtype == "i64" else C0.astype("float64")
        t0 = time.perf_counter()
        oracle.lsap(C0)
        out["oracle_ms"] = (time.perf_counter() - t0) * 1e3
    if args.tag:
        out["tag"] = args.tag
    print(json.dumps(out))
