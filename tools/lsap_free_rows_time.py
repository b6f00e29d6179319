"""dev: time the free-rows warm start and k-best against what they replace.
    python tools/lsap_free_rows_time.py [--dtype i64,f32] [--batch 16,256] [--out FILE] [--tag TEXT]
                                        [NRxNC ...]   (default: 1900x2000 250x256 64x1024 1000x2000)
    python tools/lsap_free_rows_time.py --kbest [--batch 1,64] [--k 10,100] [--out FILE] [NRxNC ...]
                                                      (default: 250x256 60x64 256x256)
Warm start.  As tools/lsap_warm_time.py: B random instances (i64: randint(0, 2^16); f32 / f64: rand * 2^16,
seed 7) are solved cold (lsap_solve_large_, duals on), which gives the state (col, v); k rows of every
instance are redrawn, k = 0, 1, 1 %, 10 % and 100 % of nr, and on the perturbed matrices the tool times
  fr_ms           lsap_warm_fr_ from the unperturbed state (both launches)
  fr_prologue_ms  ... its first launch alone (SH_FLAG_BUILD_ONLY)
  warm_ms         lsap_warm_ from the same state
  cold_ms         lsap_solve_large_ with duals
  padded_ms       lsap_warm_ on a padded copy [B, nc, nc] built beforehand (zero rows written out, col extended by
                  the free columns in ascending order); skipped where the copy would pass --padded-gib
through the C entries themselves.  HIP events, one warm-up, median of 5, ms.  kept / kept_free / searches are
means over the batch (searches = (nr - kept) + (nc - nr - kept_free); warm_kept is lsap_warm_'s).
k-best.  B instances of float64 rand * 2^16, lsap_kbest_ against lsap_kbest_fr_: ms, microseconds per
assignment, and the mean Dijkstras per child of the root's expansion and of the expansion of the root's
child nr // 2 (real rows: nr - kept; free rows add the virtual rows that hold no column in the start state).
One JSON line per record; --out appends them to FILE as well."""
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
ap.add_argument("--kbest", action="store_true")
ap.add_argument("--dtype", default="i64,f32")
ap.add_argument("--batch", default=None)
ap.add_argument("--k", default="10,100")
ap.add_argument("--padded-gib", type=float, default=12.0)
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default=None)
ap.add_argument("cases", nargs="*")
args = ap.parse_args()
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
    x = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * 65536.0
    return x.to(torch.float32) if dtype == "f32" else x


def emit(out):
    if args.tag:
        out["tag"] = args.tag
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def warm_series(nr, nc, dtype, B):
    ddt = torch.int64 if dtype == "i64" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(7)
    C = draw((B, nr, nc), dtype, g)
    stream = santa_hip.context.current_stream_handle(C.device)
    col0 = torch.empty((B, nr), dtype=torch.int32, device="cuda")
    u0 = torch.empty((B, nr), dtype=ddt, device="cuda")
    v0 = torch.empty((B, nc), dtype=ddt, device="cuda")
    cold, warm, fr = (getattr(L, f"{e}_{dtype}") for e in ("lsap_solve_large", "lsap_warm", "lsap_warm_fr"))
    assert cold(p(C), nr, nc, B, None, p(col0), None, p(u0), p(v0), 1, stream) == 0, _lib.last_error()
    col, u, v = torch.empty_like(col0), torch.empty_like(u0), torch.empty_like(v0)
    kept, kept2 = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty((B, 2), dtype=torch.int32, device="cuda")
    theta = torch.empty(B, dtype=ddt, device="cuda")
    pad = nr < nc and B * nc * nc * C.element_size() <= args.padded_gib * 2 ** 30
    if pad:  # the caller's way out today: the zero rows written out, the free columns (ascending) given to them
        taken = torch.zeros((B, nc), dtype=torch.bool, device="cuda")
        taken.scatter_(1, col0.long(), True)
        free = torch.argsort((~taken).to(torch.int8), dim=1, descending=True, stable=True)[:, :nc - nr].to(torch.int32)
        pcol0 = torch.cat([col0, free], 1).contiguous()
        pcol, pu = torch.empty_like(pcol0), torch.empty((B, nc), dtype=ddt, device="cuda")
        P = torch.zeros((B, nc, nc), dtype=C.dtype, device="cuda")
    for k in sorted({0, 1, max(1, nr // 100), max(1, nr // 10), nr}):
        D = C.clone()
        if k:  # k rows of every instance redrawn
            rows = torch.rand((B, nr), generator=g, device="cuda").argsort(1)[:, :k]
            D[torch.arange(B, device="cuda")[:, None], rows] = draw((B, k, nc), dtype, g)

        def restore():
            col.copy_(col0)
            v.copy_(v0)

        def run_fr(flags=1):
            assert fr(p(D), nr, nc, B, None, p(col), None, p(u), p(v), p(kept2), p(theta), flags, stream) == 0, \
                _lib.last_error()

        def run_warm():
            assert warm(p(D), nr, nc, B, None, p(col), None, p(u), p(v), p(kept), 1, stream) == 0, _lib.last_error()

        out = {"what": "warm", "nr": nr, "nc": nc, "B": B, "dtype": dtype, "k": k}
        out["fr_ms"] = timed(run_fr, restore)
        k2 = kept2.float().mean(0)
        out["kept"], out["kept_free"] = float(k2[0]), float(k2[1])
        out["searches"] = (nr - out["kept"]) + (nc - nr - out["kept_free"])
        out["fr_prologue_ms"] = timed(lambda: run_fr(1 | _lib.SH_FLAG_BUILD_ONLY), restore)
        out["warm_ms"] = timed(run_warm, restore)
        out["warm_kept"] = float(kept.float().mean())
        out["cold_ms"] = timed(lambda: cold(p(D), nr, nc, B, None, p(col), None, p(u), p(v), 1, stream))
        if pad:
            P[:, :nr] = D

            def restore_p():
                pcol.copy_(pcol0)
                v.copy_(v0)

            out["padded_ms"] = timed(lambda: warm(p(P), nc, nc, B, None, p(pcol), None, p(pu), p(v), p(kept), 1, stream),
                                     restore_p)
            out["padded_kept"] = float(kept.float().mean())
        emit(out)
        del D


def kbest_series(nr, nc, B):
    g = torch.Generator(device="cuda").manual_seed(7)
    C = draw((B, nr, nc), "f64", g)
    stream = santa_hip.context.current_stream_handle(C.device)
    # Dijkstras per child: the root's expansion, then the expansion of the root's child nr // 2 (of at most 4
    # instances: the count of the virtual rows' searches below is host work)
    Call, C, B = C, C[:min(B, 4)].contiguous(), min(B, 4)
    rcol, _, _, rv = santa_hip.solve_batched_large(C, duals=True)
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    none = torch.zeros((B, (nc + 63) // 64), dtype=torch.int64, device="cuda")
    per_child = {}
    for mode in (False, True):
        node = (rcol, rv, zero)
        for depth in ("root", "child"):
            ncol, nv, np_ = node
            ccol, ccost, _, cv, kept = santa_hip.murty_children_batched(C, ncol, nv, np_, none, free_rows=mode)
            alive = torch.isfinite(ccost)
            s = (nr - kept).float()
            if mode and nr < nc:  # the virtual rows that hold no column: free columns below theta
                taken = torch.zeros((B, nc), dtype=torch.bool, device="cuda").scatter_(1, ncol.long(), True)
                for b in range(B):
                    for t in range(int(np_[b]), nr):
                        open_ = torch.ones(nc, dtype=torch.bool, device="cuda")
                        open_[ncol[b, :t].long()] = False
                        tk = taken[b].clone()
                        tk[ncol[b, t]] = False  # (row t drops its pair in its own child)
                        th = nv[b][open_].max()
                        s[b, t] += (nc - nr) - min(nc - nr, int((open_ & ~tk & (nv[b] == th)).sum()))
            per_child[f"searches_{depth}_{'fr' if mode else 'default'}"] = float(s[alive].mean())
            t = nr // 2
            node = (ccol[:, t].contiguous(), cv[:, t].contiguous(), torch.full_like(zero, t))
    C, B = Call, Call.shape[0]
    for k in (int(x) for x in args.k.split(",")):
        nbytes = int(L.lsap_kbest_work_bytes(nr, nc, B, k))
        work = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
        cols = torch.empty((B, k, nr), dtype=torch.int32, device="cuda")
        costs, count = torch.empty((B, k), dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        out = {"what": "kbest", "nr": nr, "nc": nc, "B": B, "k": k, **per_child}
        for name in ("lsap_kbest_f64", "lsap_kbest_fr_f64"):
            f = getattr(L, name)
            ms = timed(lambda: f(p(C), nr, nc, B, None, k, p(cols), p(costs), p(count), p(work), nbytes, 1, stream))
            key = "fr" if "_fr_" in name else "default"
            out[key + "_ms"], out[key + "_us_per_assignment"] = ms, ms * 1000.0 / (B * k)
            out[key + "_cost_sum"] = float(costs.sum())
        emit(out)


if args.kbest:
    for case in args.cases or ["250x256", "60x64", "256x256"]:
        nr, nc = (int(x) for x in case.split("x"))
        for B in (int(b) for b in (args.batch or "1,64").split(",")):
            kbest_series(nr, nc, B)
else:
    for case in args.cases or ["1900x2000", "250x256", "64x1024", "1000x2000"]:
        nr, nc = (int(x) for x in case.split("x"))
        for dtype in args.dtype.split(","):
            for B in (int(b) for b in (args.batch or "16,256").split(",")):
                warm_series(nr, nc, dtype, B)
                torch.cuda.empty_cache()
