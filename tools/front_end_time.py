"""dev: time the batched front ends that tools/lsap_time.py does not reach (resolve_batched, the two
checks, the CSR entry, the bottleneck's witness solve and check), the Python in between included.
    python tools/front_end_time.py --tag TEXT
HIP events around the whole call, a warm-up, best and median of 3 (ms), at 8 x 8 x 1 and 64 x 64 x 16,
i64 and f32, on the previous solution of the same costs.  SANTA_HIP_PKG and SANTA_HIP_LIB select the
package and the library as in tools/lsap_time.py.  One JSON line per (entry, case, dtype): the
`entry` lines of profiles/front_end_ab.jsonl."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SANTA_HIP_PKG") or os.path.join(ROOT, "mpi-hungarian-method_amd"))
import torch  # noqa: E402
import santa_hip as S  # noqa: E402

tag = sys.argv[sys.argv.index("--tag") + 1]


def timed(call):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), statistics.median(ts)


for n, B in ((8, 1), (64, 16)):
    for dtype in ("i64", "f32"):
        g = torch.Generator(device="cuda").manual_seed(7)
        if dtype == "i64":
            C = torch.randint(0, 65536, (B, n, n), generator=g, device="cuda")
        else:
            C = (torch.rand((B, n, n), generator=g, device="cuda", dtype=torch.float64) * 65536.0).to(torch.float32)
        col, _, u, v = S.solve_batched_large(C, with_cost=False, duals=True)
        bcol, val, wit = S.solve_bottleneck_batched(C, witness=True)
        calls = {"resolve_batched": lambda: S.resolve_batched(C, col, u, v, with_cost=False),
                 "check_duals": lambda: S.check_duals(C, col, u, v),
                 "check_duals_large": lambda: S.check_duals_large(C, col, u, v),
                 "solve_bottleneck_batched(witness)": lambda: S.solve_bottleneck_batched(C, witness=True),
                 "check_bottleneck": lambda: S.check_bottleneck(C, bcol, val, wit)}
        if dtype == "f32":
            crow = torch.arange(B * n + 1, dtype=torch.int64, device="cuda") * n
            idx = torch.arange(n, dtype=torch.int32, device="cuda").repeat(B * n)
            vals = C.reshape(-1)
            calls["solve_batched_sparse"] = lambda: S.solve_batched_sparse(crow, idx, vals, shape=(B, n, n), with_cost=False)
        for entry, call in calls.items():
            best, med = timed(call)
            print(json.dumps({"entry": entry, "n": n, "B": B, "dtype": dtype, "ms": best, "median_ms": med, "tag": tag}), flush=True)
