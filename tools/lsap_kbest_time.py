"""dev: time the k best assignments (lsap_kbest_) against Murty driven from Python.
    python tools/lsap_kbest_time.py [--batch 1,64] [--k 10,100] [--out FILE] [--tag TEXT] [--reps 5]
                                    [NRxNC ...]   (default: 32x32 64x64 128x128 256x256 60x64 250x256)
For each point: B random float32 instances (rand * 2^16, seed 7), and on the same matrices
  fused_ms   lsap_kbest_f32 through the C entry, its pool allocated beforehand
  warm_ms    comparator (a): the same partition with the queue in Python (torch on the device): each
             expansion's nr masked matrices of every instance are written out and solved with
             resolve_batched from the parent's (col, v)
  cold_ms    comparator (b): the same with solve_batched_large, to show what the warm start is worth
HIP events around the whole call, one warm-up, median of --reps, ms.  Both comparators use only entries
that exist without the k-best ones.  per_rank_us is fused_ms over the assignments emitted, searches the
mean Dijkstras of a child that exists (nr - kept, from comparator (a): the fused path runs the same
prologue and the same searches), pool_bytes lsap_kbest_work_bytes, copy_bytes what one expansion of a
comparator writes as masked matrices, same whether all three returned the same costs and assignments.
256 columns with B = 64 runs k = 10 only.  One JSON line per point; --out appends them to FILE too."""
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
ap.add_argument("--batch", default="1,64")
ap.add_argument("--k", default="10,100")
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("cases", nargs="*", default=["32x32", "64x64", "128x128", "256x256", "60x64", "250x256"])
args = ap.parse_args()
L = _lib.lib()
INF = float("inf")


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timed(call):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def masked_children(C, col, pp, F):
    """The nr masked matrices of every instance's node, written out: [B * nr, nr, nc], and F_t [B, nr, nc]."""
    B, nr, nc = C.shape
    dev = C.device
    ar_r, ar_c = torch.arange(nr, device=dev), torch.arange(nc, device=dev)
    colc = col.clamp(min=0).long()
    rowof = torch.full((B, nc), nr, device=dev).scatter_(1, colc, ar_r.expand(B, nr))  # the row that holds a column
    t = ar_r.view(1, nr, 1, 1)
    i = ar_r.view(1, 1, nr, 1)
    own = colc.view(B, 1, nr, 1) == ar_c.view(1, 1, 1, nc)
    forced = rowof.view(B, 1, 1, nc) < t
    Ft = (F.view(B, 1, nc) & (ar_r.view(1, nr, 1) == pp.view(B, 1, 1))) | (colc.view(B, nr, 1) == ar_c.view(1, 1, nc))
    mask = torch.where(i < t, ~own, forced.expand(B, nr, nr, nc)) | ((i == t) & Ft.view(B, nr, 1, nc))
    return C.view(B, 1, nr, nc).expand(B, nr, nr, nc).masked_fill(mask, INF).reshape(B * nr, nr, nc), Ft


def murty_python(C, k, warm, stats=None):
    """Murty's partition in fixed row order with the pool in torch tensors: comparators (a) and (b)."""
    B, nr, nc = C.shape
    dev = C.device
    slots = 1 + (k - 1) * nr
    cost_pool = torch.full((B, slots), INF, dtype=torch.float64, device=dev)
    col_pool = torch.full((B, slots, nr), -1, dtype=torch.int32, device=dev)
    v_pool = torch.zeros((B, slots, nc), dtype=torch.float64, device=dev) if warm else None
    p_pool = torch.zeros((B, slots), dtype=torch.int64, device=dev)
    F_pool = torch.zeros((B, slots, nc), dtype=torch.bool, device=dev)
    if warm:
        col, cost, _, v = santa_hip.solve_batched_large(C, duals=True)
        v_pool[:, 0] = v
    else:
        col, cost = santa_hip.solve_batched_large(C)
    col_pool[:, 0] = col
    cost_pool[:, 0] = torch.where(col[:, 0] >= 0, cost, torch.full_like(cost, INF))
    cols = torch.full((B, k, nr), -1, dtype=torch.int32, device=dev)
    costs = torch.full((B, k), INF, dtype=torch.float64, device=dev)
    ar_b, ar_r = torch.arange(B, device=dev), torch.arange(nr, device=dev)
    u0 = torch.zeros((B * nr, nr), dtype=torch.float64, device=dev)
    for r in range(k):
        best, s = cost_pool.min(1)
        found = best < INF
        pc = torch.where(found[:, None], col_pool[ar_b, s], torch.full_like(col, -1))
        cols[:, r], costs[:, r] = pc, best
        cost_pool[ar_b, s] = INF
        if r == k - 1:
            break
        pp = torch.where(found, p_pool[ar_b, s], torch.full_like(s, -1))
        M, Ft = masked_children(C, pc, pp, F_pool[ar_b, s])
        if warm:
            ccol, ccost, _, cv, kept = santa_hip.resolve_batched(M, pc.repeat_interleave(nr, 0), u0,
                                                                 v_pool[ar_b, s].repeat_interleave(nr, 0))
            v_pool[:, 1 + r * nr:1 + (r + 1) * nr] = cv.view(B, nr, nc)
        else:
            ccol, ccost = santa_hip.solve_batched_large(M)
        exists = (pp[:, None] >= 0) & (ar_r[None, :] >= pp[:, None]) & (ccol.view(B, nr, nr)[:, :, 0] >= 0)
        cost_pool[:, 1 + r * nr:1 + (r + 1) * nr] = torch.where(exists, ccost.view(B, nr), torch.full_like(ccost.view(B, nr), INF))
        col_pool[:, 1 + r * nr:1 + (r + 1) * nr] = ccol.view(B, nr, nr)
        p_pool[:, 1 + r * nr:1 + (r + 1) * nr] = ar_r
        F_pool[:, 1 + r * nr:1 + (r + 1) * nr] = Ft
        if stats is not None and warm:
            stats.append((float(((nr - kept.view(B, nr)) * exists).sum()), float(exists.sum())))
    return cols, costs


for case in args.cases:
    nr, nc = (int(x) for x in case.split("x"))
    for B in (int(b) for b in args.batch.split(",")):
        for k in (int(x) for x in args.k.split(",")):
            if nc >= 256 and B >= 64 and k > 10:
                continue
            g = torch.Generator(device="cuda").manual_seed(7)
            C = (torch.rand((B, nr, nc), generator=g, device="cuda", dtype=torch.float64) * 65536.0).to(torch.float32)
            stream = santa_hip.context.current_stream_handle(C.device)
            nbytes = int(L.lsap_kbest_work_bytes(nr, nc, B, k))
            work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
            cols = torch.empty((B, k, nr), dtype=torch.int32, device="cuda")
            costs = torch.empty((B, k), dtype=torch.float64, device="cuda")
            count = torch.empty(B, dtype=torch.int32, device="cuda")

            def fused():
                assert L.lsap_kbest_f32(p(C), nr, nc, B, None, k, p(cols), p(costs), p(count), p(work), nbytes, 1,
                                        stream) == 0, _lib.last_error()

            out = {"nr": nr, "nc": nc, "B": B, "k": k, "dtype": "f32", "pool_bytes": nbytes,
                   "copy_bytes": B * nr * nr * nc * 4}
            out["fused_ms"] = timed(fused)
            emitted = int(count.sum())
            out["emitted"] = emitted
            out["per_rank_us"] = 1e3 * out["fused_ms"] / max(1, emitted)
            stats = []
            wcols, wcosts = murty_python(C, k, True, stats)
            ccols, ccosts = murty_python(C, k, False)
            out["searches"] = sum(a for a, _ in stats) / max(1.0, sum(b for _, b in stats))
            out["same"] = bool(torch.equal(wcosts, costs) and torch.equal(ccosts, costs) and torch.equal(wcols, cols)
                               and torch.equal(ccols, cols))
            out["warm_ms"] = timed(lambda: murty_python(C, k, True))
            out["cold_ms"] = timed(lambda: murty_python(C, k, False))
            if args.tag:
                out["tag"] = args.tag
            line = json.dumps(out)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del C, work
