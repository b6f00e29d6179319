"""dev: what the bottleneck solver's witness and certificate cost.
    python tools/lbap_witness_time.py --parent-lib PATH [--out profiles/lbap_witness.jsonl]
                                      [--n 64,256,1024,2000] [--B 16,256] [--dtypes i32,i64] [--max-gib 16]
--parent-lib: a libsanta_hip.so built from the parent commit.  Its lbap_solve_ entry is the baseline, on
the same tensors and output buffers: tools/lbap_time.py's cases (B square n x n instances, integers below
2^20 from seed 7, cast to the dtype) and its method (device events around the whole C-ABI call, one
warm-up, then the median of 5, in ms).  Per (n, B, dtype) one JSON line:
    parent_ms   the parent's lbap_solve_           solve_ms  this build's lbap_solve_ (the same kernels)
    wit_ms      lbap_solve_wit_                    check_ms  lbap_check_ on that solve's output
col and value of the three solves are compared bit for bit, and every instance must be certified
(flags == 0)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-hungarian-method_amd"))
import torch  # noqa: E402
from santa_hip import _lib  # noqa: E402
from santa_hip.context import current_stream_handle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbap_witness.jsonl"))
ap.add_argument("--n", default="64,256,1024,2000")
ap.add_argument("--B", default="16,256")
ap.add_argument("--dtypes", default="i32,i64")
ap.add_argument("--max-gib", type=float, default=16.0)
args = ap.parse_args()
DT = {"i32": torch.int32, "i64": torch.int64, "f32": torch.float32, "f64": torch.float64}
parent = ctypes.CDLL(args.parent_lib)
P = ctypes.c_void_p


def timed(call):
    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    once()
    return statistics.median(once() for _ in range(5))


def entry(lib, name):
    f = getattr(lib, name)
    f.restype, f.argtypes = _lib.SIGNATURES[name]
    return f


with open(args.out, "a") as out:
    for n in (int(x) for x in args.n.split(",")):
        for B in (int(x) for x in args.B.split(",")):
            if B * n * n * 8 > args.max_gib * 2 ** 30:
                continue
            g = torch.Generator(device="cuda").manual_seed(7)
            base = torch.randint(0, 1 << 20, (B, n, n), generator=g, device="cuda", dtype=torch.int32)
            for dt in args.dtypes.split(","):
                C = base.to(DT[dt])
                s = current_stream_handle(C.device)
                cols = [torch.empty((B, n), dtype=torch.int32, device="cuda") for _ in range(3)]
                vals = [torch.empty(B, dtype=C.dtype, device="cuda") for _ in range(3)]
                wit = torch.empty((B, n), dtype=torch.uint8, device="cuda")
                counts = torch.empty((B, 2), dtype=torch.int32, device="cuda")
                flags = torch.empty(B, dtype=torch.int32, device="cuda")
                f_parent, f_solve = entry(parent, "lbap_solve_" + dt), entry(_lib.lib(), "lbap_solve_" + dt)
                f_wit, f_check = entry(_lib.lib(), "lbap_solve_wit_" + dt), entry(_lib.lib(), "lbap_check_" + dt)

                def ok(rc):
                    assert rc == 0, rc
                rec = {"n": n, "B": B, "dtype": dt}
                rec["parent_ms"] = timed(lambda: ok(f_parent(P(C.data_ptr()), n, n, B, None, P(cols[0].data_ptr()),
                                                             P(vals[0].data_ptr()), 0, s)))
                rec["solve_ms"] = timed(lambda: ok(f_solve(P(C.data_ptr()), n, n, B, None, P(cols[1].data_ptr()),
                                                           P(vals[1].data_ptr()), 0, s)))
                rec["wit_ms"] = timed(lambda: ok(f_wit(P(C.data_ptr()), n, n, B, None, P(cols[2].data_ptr()),
                                                       P(vals[2].data_ptr()), P(wit.data_ptr()), 0, s)))
                rec["check_ms"] = timed(lambda: ok(f_check(P(C.data_ptr()), n, n, B, None, P(cols[2].data_ptr()),
                                                           P(vals[2].data_ptr()), P(wit.data_ptr()),
                                                           P(counts.data_ptr()), P(flags.data_ptr()), 0, s)))
                assert torch.equal(cols[0], cols[1]) and torch.equal(cols[0], cols[2]), (n, B, dt)
                assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2]), (n, B, dt)
                assert not flags.any() and bool((counts[:, 1] == counts[:, 0] - 1).all()), (n, B, dt)
                rec["nR_mean"] = float(counts[:, 0].float().mean())
                rec["wit_over_parent"] = rec["wit_ms"] / rec["parent_ms"]
                rec["check_over_wit"] = rec["check_ms"] / rec["wit_ms"]
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                del C
            del base
            torch.cuda.empty_cache()
