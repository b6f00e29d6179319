"""dev: time the warm start of the batched LSAP against the cold solve.
    python tools/lsap_warm_time.py [--dtype i64,f32] [--batch 16,256] [--out FILE] [--tag TEXT]
                                   [NRxNC ...]     (default: 256x256 1024x1024 2000x2000 1900x2000)
For each case: B random instances (i64: randint(0, 2^16); f32: rand * 2^16, both from seed 7) are
solved cold (lsap_solve_large_, duals on), which gives the state (col, v).  Then k rows of every
instance are redrawn, k = 0, 1, 1 %, 10 % and 100 % of nr, and on the perturbed matrices the tool times
  warm_ms      lsap_warm_ from the unperturbed state (both launches)
  prologue_ms  ... its first launch alone (SH_FLAG_BUILD_ONLY)
  cold_ms      lsap_solve_large_ with duals
  check_ms     (k = 0) lsap_check_duals_large_ on the cold result: another single pass over C
through the C entries themselves (no wrapper work inside the timed region; the in / out buffers are
restored before each run).  HIP events, one warm-up, median of 5, ms.  kept is the mean and the
minimum over the batch of the pairs the prologue kept.  One JSON line per (case, dtype, B, k);
--out appends them to FILE as well."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SANTA_HIP_PKG") or os.path.join(ROOT, "mpi-hungarian-method_amd"))
import torch  # noqa: E402
import santa_hip  # noqa: E402
from santa_hip import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="i64,f32")
ap.add_argument("--batch", default="16,256")
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default=None)
ap.add_argument("cases", nargs="*", default=["256x256", "1024x1024", "2000x2000", "1900x2000"])
args = ap.parse_args()
DT = {"i64": torch.int64, "f32": torch.float32}
L = _lib.lib()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(call, restore=lambda: None):
    restore()
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def draw(shape, dtype, g):
    if dtype == "i64":
        return torch.randint(0, 65536, shape, generator=g, device="cuda")
    return (torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * 65536.0).to(torch.float32)


for case in args.cases:
    nr, nc = (int(x) for x in case.split("x"))
    for dtype in args.dtype.split(","):
        for B in (int(b) for b in args.batch.split(",")):
            ddt = torch.int64 if dtype == "i64" else torch.float64
            g = torch.Generator(device="cuda").manual_seed(7)
            C = draw((B, nr, nc), dtype, g)
            stream = santa_hip.context.current_stream_handle(C.device)
            col0 = torch.empty((B, nr), dtype=torch.int32, device="cuda")
            u0 = torch.empty((B, nr), dtype=ddt, device="cuda")
            v0 = torch.empty((B, nc), dtype=ddt, device="cuda")
            cold, warm, check = (getattr(L, f"{e}_{dtype}") for e in ("lsap_solve_large", "lsap_warm", "lsap_check_duals_large"))
            assert cold(p(C), nr, nc, B, None, p(col0), None, p(u0), p(v0), 1, stream) == 0, _lib.last_error()
            col, u, v = torch.empty_like(col0), torch.empty_like(u0), torch.empty_like(v0)
            kept = torch.empty(B, dtype=torch.int32, device="cuda")
            slack, cflags = torch.empty((B, 3), dtype=ddt, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
            for k in sorted({0, 1, max(1, nr // 100), max(1, nr // 10), nr}):
                D = C.clone()
                if k:  # k rows of every instance redrawn
                    rows = torch.rand((B, nr), generator=g, device="cuda").argsort(1)[:, :k]
                    D[torch.arange(B, device="cuda")[:, None], rows] = draw((B, k, nc), dtype, g)

                def restore():
                    col.copy_(col0)
                    v.copy_(v0)

                def run_warm(flags=1):
                    assert warm(p(D), nr, nc, B, None, p(col), None, p(u), p(v), p(kept), flags, stream) == 0, _lib.last_error()

                out = {"nr": nr, "nc": nc, "B": B, "dtype": dtype, "k": k}
                out["warm_ms"] = timed(run_warm, restore)
                out["kept_mean"], out["kept_min"] = float(kept.float().mean()), int(kept.min())
                out["prologue_ms"] = timed(lambda: run_warm(1 | _lib.SH_FLAG_BUILD_ONLY), restore)
                out["cold_ms"] = timed(lambda: cold(p(D), nr, nc, B, None, p(col), None, p(u), p(v), 1, stream))
                if k == 0:
                    out["check_ms"] = timed(lambda: check(p(D), nr, nc, B, None, p(col), p(u), p(v), p(slack), p(cflags), stream))
                if args.tag:
                    out["tag"] = args.tag
                line = json.dumps(out)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
            del C, D
