"""dev: time the batched bottleneck assignment, both designs and four dtypes, with the min-sum
solver of another build of the library beside it as context.
    python tools/lbap_time.py [--out profiles/lbap.jsonl] [--n 64,256,1024,2000,4096] [--B 16,256,4096]
                              [--dtypes i32,i64,f32,f64] [--context-lib PATH] [--max-gib 16] [--slow-s 4]
Each case is B square n x n instances, integers drawn below 2^20 from seed 7 on the device and cast to
the dtype, so that the 32-bit-key dtypes (i32, f32) and the 64-bit-key ones (i64, f64) solve the same
values and return the same col.  Timed with device events around the whole solve_bottleneck_batched
call: one warm-up, then the median of 5 (ms), for the forced multi-wave design and, up to 1024
columns, the forced one-wave one and the default.  A case whose tensor exceeds --max-gib is left out; one
whose warm-up takes longer than --slow-s seconds is recorded from that single run ("reps": 1).
--context-lib: a libsanta_hip.so of another commit (the parent's).  Its lsap_solve_large_ entry is
timed the same way on the same tensor ("lsap_large_ms"): context only -- a min-sum search takes
other steps than a bottleneck search on the same matrix, so the ratio says nothing about either.
One JSON line per (n, B, dtype), appended to --out.  SANTA_HIP_PKG and SANTA_HIP_LIB select the
package and the library as in tools/lsap_time.py."""
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
from santa_hip.context import current_stream_handle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbap.jsonl"))
ap.add_argument("--n", default="64,256,1024,2000,4096")
ap.add_argument("--B", default="16,256,4096")
ap.add_argument("--dtypes", default="i32,i64,f32,f64")
ap.add_argument("--context-lib", default=None)
ap.add_argument("--max-gib", type=float, default=16.0)
ap.add_argument("--slow-s", type=float, default=4.0)
args = ap.parse_args()
DT = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64}
DESIGNS = {"default": 0, "mw": _lib.SH_FLAG_LBAP_MW, "sw": _lib.SH_FLAG_LBAP_SW}
ctx = ctypes.CDLL(args.context_lib) if args.context_lib else None


def timed(call, slow_s):
    """(median ms, reps): one warm-up, then 5 runs; the warm-up alone when it is slow."""
    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    warm = once()
    if warm > slow_s * 1e3:
        return warm, 1
    return statistics.median(once() for _ in range(5)), 5


def context_call(C, suffix):
    B, n, _ = C.shape
    col = torch.empty((B, n), dtype=torch.int32, device=C.device)
    f = getattr(ctx, "lsap_solve_large_" + suffix)
    f.restype, f.argtypes = _lib.SIGNATURES["lsap_solve_large_" + suffix]
    p = ctypes.c_void_p

    def call():
        rc = f(p(C.data_ptr()), n, n, B, None, p(col.data_ptr()), None, None, None, _lib.SH_COMPAT_TIEBREAK,
               current_stream_handle(C.device))
        assert rc == 0, rc
    return call


with open(args.out, "a") as out:
    for n in (int(x) for x in args.n.split(",")):
        for B in (int(x) for x in args.B.split(",")):
            g = torch.Generator(device="cuda").manual_seed(7)
            if B * n * n * 8 > args.max_gib * 2 ** 30:
                continue
            base = torch.randint(0, 1 << 20, (B, n, n), generator=g, device="cuda", dtype=torch.int32)
            cols = {}
            for dt in args.dtypes.split(","):
                C = base.to(DT[dt])
                rec = {"n": n, "B": B, "dtype": dt, "key_bits": 64 if dt.endswith("64") else 32}
                for name, flags in DESIGNS.items():
                    if name != "mw" and n > _lib.SH_MAX_N:  # (one design there: the default is the same launch)
                        continue
                    res = {}

                    def call():
                        res["col"], _ = santa_hip.solve_bottleneck_batched(C, with_value=False, flags=flags)
                    rec[name + "_ms"], reps = timed(call, args.slow_s)
                    if reps != 5:
                        rec[name + "_reps"] = reps
                    cols.setdefault("col", res["col"])
                    assert torch.equal(cols["col"], res["col"]), (n, B, dt, name)  # one answer, every design and dtype
                if ctx is not None:
                    rec["lsap_large_ms"], reps = timed(context_call(C, dt), args.slow_s)
                    if reps != 5:
                        rec["lsap_large_reps"] = reps
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                del C
            del base
            torch.cuda.empty_cache()
