"""dev: time the k best assignments on the CSR (lsap_kbest_csr_) against its two alternatives.
    python tools/lsap_kbest_sparse_time.py [--batch 1,64] [--k 10] [--density 0.01,0.05,0.40] [--out FILE]
                                           [--tag TEXT] [--reps 5] [--b-cap ENTRIES] [NRxNC ...]
                                           (default: 64x64 58x64 256x256 250x256 1024x1024 1018x1024)
For each point: B band instances (the diagonal plus random entries at the density, float32 values
rand * 2^16, seed 7) as one CSR batch, and on the same instances
  fused_ms   lsap_kbest_csr_f32 through the C entry, its work buffer allocated beforehand
  dense_ms   comparator (a): lsap_kbest_f32 on the densification, built beforehand (the time to densify
             is not counted), its pool allocated beforehand
  python_ms  comparator (b): the same partition with the queue in Python (torch on the device): each
             expansion's nr masked CSRs of every instance are written out and solved with
             resolve_batched_sparse from the parent's (col, v).  An expansion writes B * nr * nnz_b
             entries before masking; above --b-cap (default 2^26) the comparator is not run (null).
HIP events around the whole call, one warm-up, median of --reps, ms.  Both comparators use only entries
that exist without the sparse k-best ones.  csr_bytes is the batch (int64 indptr, int32 indices, float32
values), dense_bytes its densification, pool_bytes lsap_kbest_work_bytes (both paths), work_bytes
lsap_kbest_csr_work_bytes (the pool and the CSR's words), same whether all that ran returned the same
cols, costs and count.  One JSON line per point; --out appends them to FILE too
(profiles/lsap_kbest_sparse.jsonl)."""
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
ap.add_argument("--k", default="10")
ap.add_argument("--density", default="0.01,0.05,0.40")
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--b-cap", type=int, default=1 << 26)
ap.add_argument("cases", nargs="*", default=["64x64", "58x64", "256x256", "250x256", "1024x1024", "1018x1024"])
args = ap.parse_args()
L = _lib.lib()
INF = float("inf")


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


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


def band(B, nr, nc, density, g):
    """-> (crow int64 [B * nr + 1], idx int32, val float32, dense float32 [B, nr, nc])."""
    P = torch.rand((B, nr, nc), generator=g, device="cuda") < density
    ar = torch.arange(nr, device="cuda")
    P[:, ar, ar] = True
    V = (torch.rand((B, nr, nc), generator=g, device="cuda", dtype=torch.float64) * 65536.0).to(torch.float32)
    dense = torch.where(P, V, torch.full_like(V, INF))
    crow = torch.zeros(B * nr + 1, dtype=torch.int64, device="cuda")
    crow[1:] = P.view(B * nr, nc).sum(1).cumsum(0)
    idx = P.view(B * nr, nc).nonzero()[:, 1].to(torch.int32)
    return crow, idx, V[P], dense


def masked_children_csr(crow, idx, val, B, nr, nc, col, pp, F):
    """The nr masked CSRs of every instance's node, written out as one batch of B * nr instances."""
    dev = crow.device
    ar_r = torch.arange(nr, device=dev)
    colc = col.clamp(min=0).long()
    rowof = torch.full((B, nc), nr, device=dev).scatter_(1, colc, ar_r.expand(B, nr))  # the row that holds a column
    start = crow[::nr][:B]
    cnt = crow[nr::nr] - start                                      # entries of an instance
    cc = cnt.repeat_interleave(nr)                                  # ... of a child, before masking
    cstart = cc.cumsum(0) - cc
    cid = torch.repeat_interleave(torch.arange(B * nr, device=dev), cc)
    src = start[cid // nr] + (torch.arange(cid.numel(), device=dev) - cstart[cid])
    erow = torch.repeat_interleave(torch.arange(B * nr, device=dev), crow[1:] - crow[:-1])
    b, t, i, j = cid // nr, cid % nr, erow[src] % nr, idx[src].long()
    Ft = (F[b, j] & (t == pp[b])) | (colc[b, t] == j)
    keep = torch.where(i < t, colc[b, i] == j, ~(rowof[b, j] < t) & ~((i == t) & Ft))
    rows = torch.bincount((cid * nr + i)[keep], minlength=B * nr * nr)
    ccrow = torch.zeros(B * nr * nr + 1, dtype=torch.int64, device=dev)
    ccrow[1:] = rows.cumsum(0)
    Ft_full = (F.view(B, 1, nc) & (ar_r.view(1, nr, 1) == pp.view(B, 1, 1))) | \
        (colc.view(B, nr, 1) == torch.arange(nc, device=dev).view(1, 1, nc))
    return ccrow, idx[src][keep], val[src][keep], Ft_full


def murty_python(crow, idx, val, B, nr, nc, k):
    """Murty's partition in fixed row order with the pool in torch tensors: comparator (b)."""
    dev = crow.device
    slots = 1 + (k - 1) * nr
    cost_pool = torch.full((B, slots), INF, dtype=torch.float64, device=dev)
    col_pool = torch.full((B, slots, nr), -1, dtype=torch.int32, device=dev)
    v_pool = torch.zeros((B, slots, nc), dtype=torch.float64, device=dev)
    p_pool = torch.zeros((B, slots), dtype=torch.int64, device=dev)
    F_pool = torch.zeros((B, slots, nc), dtype=torch.bool, device=dev)
    col, cost, _, v = santa_hip.solve_batched_sparse(crow, idx, val, (B, nr, nc), duals=True, validate=False)
    v_pool[:, 0] = v
    col_pool[:, 0] = col
    cost_pool[:, 0] = torch.where(col[:, 0] >= 0, cost, torch.full_like(cost, INF))
    cols = torch.full((B, k, nr), -1, dtype=torch.int32, device=dev)
    costs = torch.full((B, k), INF, dtype=torch.float64, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    ar_b, ar_r = torch.arange(B, device=dev), torch.arange(nr, device=dev)
    u0 = torch.zeros((B * nr, nr), dtype=torch.float64, device=dev)
    for r in range(k):
        best, s = cost_pool.min(1)
        found = best < INF
        pc = torch.where(found[:, None], col_pool[ar_b, s], torch.full_like(col, -1))
        cols[:, r], costs[:, r] = pc, best
        count += found.to(torch.int32)
        cost_pool[ar_b, s] = INF
        if r == k - 1:
            break
        pp = torch.where(found, p_pool[ar_b, s], torch.full_like(s, -1))
        ccrow, cidx, cval, Ft = masked_children_csr(crow, idx, val, B, nr, nc, pc, pp, F_pool[ar_b, s])
        ccol, ccost, _, cv, _ = santa_hip.resolve_batched_sparse(
            ccrow, cidx, cval, (B * nr, nr, nc), pc.repeat_interleave(nr, 0), u0,
            v_pool[ar_b, s].repeat_interleave(nr, 0), validate=False)
        v_pool[:, 1 + r * nr:1 + (r + 1) * nr] = cv.view(B, nr, nc)
        exists = (pp[:, None] >= 0) & (ar_r[None, :] >= pp[:, None]) & (ccol.view(B, nr, nr)[:, :, 0] >= 0)
        cost_pool[:, 1 + r * nr:1 + (r + 1) * nr] = torch.where(exists, ccost.view(B, nr),
                                                                torch.full_like(ccost.view(B, nr), INF))
        col_pool[:, 1 + r * nr:1 + (r + 1) * nr] = ccol.view(B, nr, nr)
        p_pool[:, 1 + r * nr:1 + (r + 1) * nr] = ar_r
        F_pool[:, 1 + r * nr:1 + (r + 1) * nr] = Ft
    return cols, costs, count


for case in args.cases:
    nr, nc = (int(x) for x in case.split("x"))
    for density in (float(x) for x in args.density.split(",")):
        for B in (int(b) for b in args.batch.split(",")):
            for k in (int(x) for x in args.k.split(",")):
                g = torch.Generator(device="cuda").manual_seed(7)
                crow, idx, val, dense = band(B, nr, nc, density, g)
                nnz = int(idx.numel())
                stream = santa_hip.context.current_stream_handle(crow.device)
                pool_bytes = int(L.lsap_kbest_work_bytes(nr, nc, B, k))
                work_bytes = int(L.lsap_kbest_csr_work_bytes(nr, nc, B, k))
                work = torch.empty(work_bytes // 8, dtype=torch.int64, device="cuda")
                outs = [(torch.empty((B, k, nr), dtype=torch.int32, device="cuda"),
                         torch.empty((B, k), dtype=torch.float64, device="cuda"),
                         torch.empty(B, dtype=torch.int32, device="cuda")) for _ in range(2)]

                def fused():
                    cols, costs, count = outs[0]
                    assert L.lsap_kbest_csr_f32(p(crow), p(idx), p(val), nr, nc, B, None, k, p(cols), p(costs),
                                                p(count), p(work), work_bytes, 1, stream) == 0, _lib.last_error()

                def dense_kbest():
                    cols, costs, count = outs[1]
                    assert L.lsap_kbest_f32(p(dense), nr, nc, B, None, k, p(cols), p(costs), p(count), p(work),
                                            pool_bytes, 1, stream) == 0, _lib.last_error()

                out = {"nr": nr, "nc": nc, "B": B, "k": k, "density": density, "nnz": nnz, "dtype": "f32",
                       "csr_bytes": 8 * (B * nr + 1) + 8 * nnz, "dense_bytes": 4 * B * nr * nc,
                       "pool_bytes": pool_bytes, "work_bytes": work_bytes}
                out["fused_ms"] = timed(fused)
                out["dense_ms"] = timed(dense_kbest)
                same = all(torch.equal(a, b) for a, b in zip(*outs))
                out["emitted"] = int(outs[0][2].sum())
                if nnz * nr <= args.b_cap:
                    pc = murty_python(crow, idx, val, B, nr, nc, k)
                    same = same and all(torch.equal(a, b) for a, b in zip(pc, outs[0]))
                    out["python_ms"] = timed(lambda: murty_python(crow, idx, val, B, nr, nc, k))
                else:
                    out["python_ms"] = None
                out["python_entries"] = nnz * nr
                out["same"] = bool(same)
                out["dense_over_fused"] = out["dense_ms"] / out["fused_ms"]
                out["python_over_fused"] = out["python_ms"] / out["fused_ms"] if out["python_ms"] else None
                if args.tag:
                    out["tag"] = args.tag
                line = json.dumps(out)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
                del crow, idx, val, dense, work, outs
