"""dev: time free rows on sparse (CSR) costs.
    python tools/lsap_free_rows_sparse_time.py [--density 0.01,0.05,0.4] [--batch 64] [--out FILE] [NRxNC ...]
    python tools/lsap_free_rows_sparse_time.py --kbest [--density 0.05] [--batch 1,64] [--k 10] [--out FILE] [NRxNC ...]
Warm start (default cases 250x256 1018x1024 1900x2000 64x1024).  B instances whose pattern is the diagonal
plus each other entry with the given probability (the band_ patterns of tools/lsap_warm_sparse_time.py),
float64 values that are random integers below 2^16 from seed 7, are solved cold (lsap_solve_csr_ with
duals), which gives the state (col, v).  Then the values of k rows of every instance are redrawn with the
pattern kept, k = 0, 1, 1 %, 10 % and 100 % of nr, and on the perturbed batch the tool times
  fr_prologue_ms  lsap_warm_fr_csr_ with SH_FLAG_BUILD_ONLY (the pass over the CSR and the prologue)
  fr_ms           lsap_warm_fr_csr_ from the unperturbed state (all three launches)
  warm_ms         lsap_warm_csr_ from the same state
  cold_ms         lsap_solve_csr_ with duals
  dense_fr_ms     lsap_warm_fr_f64 on a densification built beforehand, where it fits in --dense-gb (8)
through the C entries themselves (the in / out buffers are restored before each run).  HIP events; every
variant runs once as a warm-up, then the variants alternate for 5 rounds and each reports its median, ms.
kept / kept_free / searches are means over the batch (searches = (nr - kept) + (nc - nr - kept_free));
warm_kept is lsap_warm_csr_'s.  Every cell checks that the free-rows cost equals the cold solve's and, where
the dense run exists, that col and both counts equal its.
k-best (default cases 60x64 250x256 1018x1024).  The same patterns with generic float64 values rand * 2^16:
lsap_kbest_fr_csr_ against lsap_kbest_csr_ and against lsap_kbest_fr_f64 on the densification: ms,
microseconds per assignment (ms / (B k)) and the summed costs; searches per child are means over the
children of the root and over the children of the root's child nr // 2 of the first instance, counted from
`kept` and, with free rows, from the virtual rows the start state leaves without a column.
One JSON line per cell; --out appends them to FILE as well (default profiles/lsap_free_rows_sparse.jsonl)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SANTA_HIP_PKG") or os.path.join(ROOT, "mpi-hungarian-method_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import santa_hip  # noqa: E402
from santa_hip import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kbest", action="store_true")
ap.add_argument("--density", default=None)
ap.add_argument("--batch", default=None)
ap.add_argument("--k", default="10")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsap_free_rows_sparse.jsonl"))
ap.add_argument("--tag", default=None)
ap.add_argument("--dense-gb", type=float, default=8.0)
ap.add_argument("cases", nargs="*")
args = ap.parse_args()
L = _lib.lib()
TIE, BUILD_ONLY = _lib.SH_COMPAT_TIEBREAK, _lib.SH_FLAG_BUILD_ONLY


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ok(rc):
    assert rc == 0, _lib.last_error()


def timed(variants):
    """{name: median ms} of {name: (call, restore)}: one warm-up each, then 5 alternating rounds."""
    for call, restore in variants.values():
        restore()
        call()
    torch.cuda.synchronize()
    ts = {name: [] for name in variants}
    for _ in range(5):
        for name, (call, restore) in variants.items():
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: statistics.median(t) for name, t in ts.items()}


def pattern(B, nr, nc, density, g):
    """(crow int64 [B * nr + 1], idx int32 [nnz], row int64 [nnz]) of the diagonal plus random entries."""
    counts, idx = [], []
    diag = torch.zeros((nr, nc), dtype=torch.bool, device="cuda")
    diag[torch.arange(nr), torch.arange(nr)] = True
    for _ in range(B):
        P = (torch.rand((nr, nc), generator=g, device="cuda") < density) | diag
        counts.append(P.sum(1))
        idx.append(P.nonzero()[:, 1].to(torch.int32))
    counts = torch.cat(counts)
    crow = torch.zeros(B * nr + 1, dtype=torch.int64, device="cuda")
    crow[1:] = counts.cumsum(0)
    row = torch.repeat_interleave(torch.arange(B * nr, device="cuda"), counts)
    return crow, torch.cat(idx), row


def densified(B, nr, nc, row, idx, val):
    D = torch.full((B * nr, nc), float("inf"), dtype=torch.float64, device="cuda")
    D[row, idx.long()] = val
    return D


def emit(out):
    if args.tag:
        out["tag"] = args.tag
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def warm_series(nr, nc, density, B):
    g = torch.Generator(device="cuda").manual_seed(7)
    crow, idx, row = pattern(B, nr, nc, density, g)
    nnz = idx.numel()
    val0 = torch.randint(0, 65536, (nnz,), generator=g, device="cuda").double()
    stream = santa_hip.context.current_stream_handle(val0.device)
    nbytes = int(L.lsap_csr_work_bytes(nr, nc, B))
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    new = lambda *shape, dt=torch.float64: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
    col0, u0, v0 = new(B, nr, dt=torch.int32), new(B, nr), new(B, nc)
    cold, warm, fr, dense_fr = L.lsap_solve_csr_f64, L.lsap_warm_csr_f64, L.lsap_warm_fr_csr_f64, L.lsap_warm_fr_f64
    ok(cold(p(crow), p(idx), p(val0), nr, nc, B, None, p(col0), None, p(u0), p(v0), p(work), nbytes, TIE, stream))
    assert bool((col0 >= 0).all()), "the pattern is feasible by construction"
    col, u, v, cost = new(B, nr, dt=torch.int32), new(B, nr), new(B, nc), new(B)
    wcol, wu, wv = new(B, nr, dt=torch.int32), new(B, nr), new(B, nc)
    ccol, cu, cv, ccost = new(B, nr, dt=torch.int32), new(B, nr), new(B, nc), new(B)
    kept, theta, wkept = new(B, 2, dt=torch.int32), new(B), new(B, dt=torch.int32)
    dense = B * nr * nc * 8 <= args.dense_gb * (1 << 30)
    if dense:
        dcol, du, dv, dkept, dtheta = new(B, nr, dt=torch.int32), new(B, nr), new(B, nc), new(B, 2, dt=torch.int32), new(B)
    for k in sorted({0, 1, max(1, nr // 100), max(1, nr // 10), nr}):
        val = val0.clone()
        if k:  # the values of k rows of every instance redrawn, the pattern kept
            pick = torch.rand((B, nr), generator=g, device="cuda").argsort(1)[:, :k]
            sel = torch.zeros((B, nr), dtype=torch.bool, device="cuda")
            sel[torch.arange(B, device="cuda")[:, None], pick] = True
            val = torch.where(sel.view(-1)[row], torch.randint(0, 65536, (nnz,), generator=g, device="cuda").double(), val)

        def restore():
            col.copy_(col0)
            v.copy_(v0)

        def restore_warm():
            wcol.copy_(col0)
            wv.copy_(v0)

        def run_fr(flags=0):
            ok(fr(p(crow), p(idx), p(val), nr, nc, B, None, p(col), p(cost), p(u), p(v), p(kept), p(theta), p(work),
                  nbytes, TIE | flags, stream))

        def run_warm():
            ok(warm(p(crow), p(idx), p(val), nr, nc, B, None, p(wcol), None, p(wu), p(wv), p(wkept), p(work), nbytes,
                    TIE, stream))

        def run_cold():
            ok(cold(p(crow), p(idx), p(val), nr, nc, B, None, p(ccol), p(ccost), p(cu), p(cv), p(work), nbytes, TIE,
                    stream))

        variants = {"fr_prologue_ms": (lambda: run_fr(BUILD_ONLY), restore), "fr_ms": (run_fr, restore),
                    "warm_ms": (run_warm, restore_warm), "cold_ms": (run_cold, lambda: None)}
        if dense:
            D = densified(B, nr, nc, row, idx, val)

            def restore_dense():
                dcol.copy_(col0)
                dv.copy_(v0)

            def run_dense():
                ok(dense_fr(p(D), nr, nc, B, None, p(dcol), None, p(du), p(dv), p(dkept), p(dtheta), TIE, stream))

            variants["dense_fr_ms"] = (run_dense, restore_dense)
        out = {"what": "warm", "nr": nr, "nc": nc, "B": B, "density": density, "nnz": nnz, "k": k}
        out.update(timed(variants))
        restore()
        run_fr(BUILD_ONLY)   # the counts are the start state's
        out["kept"], out["kept_free"] = (float(x) for x in kept.float().mean(0))
        out["searches"] = (nr - out["kept"]) + (nc - nr - out["kept_free"])
        out["warm_kept"] = float(wkept.float().mean())
        restore()
        run_fr()
        out["optimal"] = bool(torch.equal(cost, ccost))   # (integer values: every sum is exact)
        assert out["optimal"]
        if dense:
            out["equals_dense"] = bool(torch.equal(col, dcol))
            assert out["equals_dense"]
            del D
        for a, b_ in (("cold", "fr"), ("warm", "fr")):
            out[f"{a}_over_{b_}"] = out[a + "_ms"] / out[b_ + "_ms"]
        if dense:
            out["fr_over_dense_fr"] = out["fr_ms"] / out["dense_fr_ms"]
        emit(out)


def searches_per_child(crow, idx, val, nr, nc):
    """Means over the children of the root and of the root's child nr // 2 of the first instance."""
    crow1, n1 = crow[:nr + 1].clone(), int(crow[nr])
    tri = (crow1, idx[:n1], val[:n1], (1, nr, nc))
    rcol, _, _, rv = santa_hip.solve_batched_sparse(*tri, duals=True)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    none = torch.zeros((1, (nc + 63) // 64), dtype=torch.int64, device="cuda")
    out = {}
    for mode in (False, True):
        node = (rcol, rv, zero)
        for depth in ("root", "child"):
            ncol, nv, np_ = node
            ccol, ccost, _, cv, kept = santa_hip.murty_children_batched_sparse(*tri, ncol, nv, np_, none, free_rows=mode)
            alive = torch.isfinite(ccost[0]).cpu().numpy()
            s = (nr - kept[0]).cpu().numpy().astype(float)
            if mode and nr < nc:  # the virtual rows that hold no column: free columns below theta
                c, vv = ncol[0].cpu().numpy(), nv[0].cpu().numpy()
                for t in range(int(np_[0]), nr):
                    open_ = np.ones(nc, dtype=bool)
                    open_[c[:t]] = False
                    taken = np.zeros(nc, dtype=bool)
                    taken[c] = True
                    taken[c[t]] = False  # (row t drops its pair in its own child)
                    th = vv[open_].max()
                    s[t] += (nc - nr) - min(nc - nr, int((open_ & ~taken & (vv == th)).sum()))
            out[f"searches_{depth}_{'fr' if mode else 'default'}"] = float(s[alive].mean()) if alive.any() else None
            t = nr // 2
            node = (ccol[:, t].contiguous(), cv[:, t].contiguous(), torch.full_like(zero, t))
    return out


def kbest_series(nr, nc, density, B):
    g = torch.Generator(device="cuda").manual_seed(7)
    crow, idx, row = pattern(B, nr, nc, density, g)
    val = torch.rand(idx.numel(), generator=g, device="cuda", dtype=torch.float64) * 65536.0
    stream = santa_hip.context.current_stream_handle(val.device)
    per_child = searches_per_child(crow, idx, val, nr, nc)
    D = densified(B, nr, nc, row, idx, val)
    for k in (int(x) for x in args.k.split(",")):
        nbytes = int(L.lsap_kbest_csr_work_bytes(nr, nc, B, k))
        work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
        cols = torch.empty((B, k, nr), dtype=torch.int32, device="cuda")
        costs, count = torch.empty((B, k), dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        dbytes = int(L.lsap_kbest_work_bytes(nr, nc, B, k))

        def sparse(f):
            return lambda: ok(f(p(crow), p(idx), p(val), nr, nc, B, None, k, p(cols), p(costs), p(count), p(work), nbytes,
                                TIE, stream))

        variants = {"fr_ms": (sparse(L.lsap_kbest_fr_csr_f64), lambda: None),
                    "default_ms": (sparse(L.lsap_kbest_csr_f64), lambda: None),
                    "dense_fr_ms": (lambda: ok(L.lsap_kbest_fr_f64(p(D), nr, nc, B, None, k, p(cols), p(costs), p(count),
                                                                   p(work), dbytes, TIE, stream)), lambda: None)}
        out = {"what": "kbest", "nr": nr, "nc": nc, "B": B, "k": k, "density": density, **per_child}
        out.update(timed(variants))
        for name, (call, _) in variants.items():
            call()
            torch.cuda.synchronize()
            out[name[:-3] + "_cost_sum"] = float(costs[torch.isfinite(costs)].sum())
            out[name[:-3] + "_us_per_assignment"] = out[name] * 1000.0 / (B * k)
        out["default_over_fr"] = out["default_ms"] / out["fr_ms"]
        out["fr_over_dense_fr"] = out["fr_ms"] / out["dense_fr_ms"]
        emit(out)


if args.kbest:
    for case in args.cases or ["60x64", "250x256", "1018x1024"]:
        nr, nc = (int(x) for x in case.split("x"))
        for density in (float(d) for d in (args.density or "0.05").split(",")):
            for B in (int(b) for b in (args.batch or "1,64").split(",")):
                kbest_series(nr, nc, density, B)
                torch.cuda.empty_cache()
else:
    for case in args.cases or ["250x256", "1018x1024", "1900x2000", "64x1024"]:
        nr, nc = (int(x) for x in case.split("x"))
        for density in (float(d) for d in (args.density or "0.01,0.05,0.4").split(",")):
            for B in (int(b) for b in (args.batch or "64").split(",")):
                warm_series(nr, nc, density, B)
                torch.cuda.empty_cache()
