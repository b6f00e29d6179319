"""dev: time the warm start on sparse (CSR) costs against the cold sparse solve and the dense warm
start.
    python tools/lsap_warm_sparse_time.py [--density 0.01,0.05,0.4] [--batch 16,256] [--out FILE] [--tag TEXT]
                                          [NRxNC ...]     (default: 1024x1024 4096x4096 1900x2000)
For each case: B instances whose pattern is the diagonal plus each other entry with the given
probability (the test families' band_ patterns: feasible by construction), float64 values that are
random integers below 2^16 from seed 7 (every sum is exact, so the certificate's equalities hold),
are solved cold (lsap_solve_csr_, duals on), which gives the state (col, v).  Then the values of k rows of every instance are redrawn with the pattern kept, k = 0, 1, 1 %, 10 % and 100 % of
nr, and on the perturbed batch the tool times
  prep_ms      the pass over the CSR that fills d_work (lsap_solve_csr_ with SH_FLAG_BUILD_ONLY)
  prologue_ms  ... plus the warm prologue (lsap_warm_csr_ with SH_FLAG_BUILD_ONLY)
  warm_ms      lsap_warm_csr_ from the unperturbed state (all three launches)
  cold_ms      lsap_solve_csr_ with duals
  dense_warm_ms  lsap_warm_f64 on the densification, where B * nr * nc * 8 bytes fit in --dense-gb (8)
through the C entries themselves (no wrapper work inside the timed region; the in / out buffers are
restored before each run).  HIP events; every variant runs once as a warm-up, then the variants
alternate for 5 rounds and each reports its median, ms.  kept_mean is the mean over the batch of
the pairs the prologue kept.  Every cell checks check_duals_sparse(...) flags == 0 on the warm result
and, where the dense run exists, that col and kept equal its.  One JSON line per cell; --out appends
them to FILE as well (default profiles/lsap_warm_sparse.jsonl)."""
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
ap.add_argument("--density", default="0.01,0.05,0.4")
ap.add_argument("--batch", default="16,256")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsap_warm_sparse.jsonl"))
ap.add_argument("--tag", default=None)
ap.add_argument("--dense-gb", type=float, default=8.0)
ap.add_argument("cases", nargs="*", default=["1024x1024", "4096x4096", "1900x2000"])
args = ap.parse_args()
L = _lib.lib()
TIE, BUILD_ONLY = _lib.SH_COMPAT_TIEBREAK, _lib.SH_FLAG_BUILD_ONLY


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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
    for _ in range(B):  # (one instance at a time: a 4096 x 4096 batch of masks would not fit)
        P = (torch.rand((nr, nc), generator=g, device="cuda") < density) | diag
        counts.append(P.sum(1))
        idx.append(P.nonzero()[:, 1].to(torch.int32))
    counts = torch.cat(counts)
    crow = torch.zeros(B * nr + 1, dtype=torch.int64, device="cuda")
    crow[1:] = counts.cumsum(0)
    row = torch.repeat_interleave(torch.arange(B * nr, device="cuda"), counts)
    return crow, torch.cat(idx), row


def ok(rc):
    assert rc == 0, _lib.last_error()


for case in args.cases:
    nr, nc = (int(x) for x in case.split("x"))
    for density in (float(d) for d in args.density.split(",")):
        for B in (int(b) for b in args.batch.split(",")):
            g = torch.Generator(device="cuda").manual_seed(7)
            crow, idx, row = pattern(B, nr, nc, density, g)
            nnz = idx.numel()
            val0 = torch.randint(0, 65536, (nnz,), generator=g, device="cuda").double()
            stream = santa_hip.context.current_stream_handle(val0.device)
            nbytes = int(L.lsap_csr_work_bytes(nr, nc, B))
            work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            col0 = torch.empty((B, nr), dtype=torch.int32, device="cuda")
            u0 = torch.empty((B, nr), dtype=torch.float64, device="cuda")
            v0 = torch.empty((B, nc), dtype=torch.float64, device="cuda")
            cold, warm, dense_warm = L.lsap_solve_csr_f64, L.lsap_warm_csr_f64, L.lsap_warm_f64
            ok(cold(p(crow), p(idx), p(val0), nr, nc, B, None, p(col0), None, p(u0), p(v0), p(work), nbytes, TIE, stream))
            assert bool((col0 >= 0).all()), "the pattern is feasible by construction"
            col, u, v = torch.empty_like(col0), torch.empty_like(u0), torch.empty_like(v0)
            ccol, cu, cv = torch.empty_like(col0), torch.empty_like(u0), torch.empty_like(v0)
            kept = torch.empty(B, dtype=torch.int32, device="cuda")
            dense = B * nr * nc * 8 <= args.dense_gb * (1 << 30)
            if dense:
                dcol, du, dv = torch.empty_like(col0), torch.empty_like(u0), torch.empty_like(v0)
                dkept = torch.empty_like(kept)
            for k in sorted({0, 1, max(1, nr // 100), max(1, nr // 10), nr}):
                val = val0.clone()
                if k:  # the values of k rows of every instance redrawn, the pattern kept
                    pick = torch.rand((B, nr), generator=g, device="cuda").argsort(1)[:, :k]
                    sel = torch.zeros((B, nr), dtype=torch.bool, device="cuda")
                    sel[torch.arange(B, device="cuda")[:, None], pick] = True
                    new = torch.randint(0, 65536, (nnz,), generator=g, device="cuda").double()
                    val = torch.where(sel.view(-1)[row], new, val)

                def restore():
                    col.copy_(col0)
                    v.copy_(v0)

                def run_warm(flags=0):
                    ok(warm(p(crow), p(idx), p(val), nr, nc, B, None, p(col), None, p(u), p(v), p(kept), p(work), nbytes,
                            TIE | flags, stream))

                def run_cold(flags=0):
                    ok(cold(p(crow), p(idx), p(val), nr, nc, B, None, p(ccol), None, p(cu), p(cv), p(work), nbytes,
                            TIE | flags, stream))

                variants = {"prep_ms": (lambda: run_cold(BUILD_ONLY), lambda: None),
                            "prologue_ms": (lambda: run_warm(BUILD_ONLY), restore),
                            "warm_ms": (run_warm, restore),
                            "cold_ms": (run_cold, lambda: None)}
                if dense:
                    D = torch.full((B * nr, nc), float("inf"), dtype=torch.float64, device="cuda")
                    D[row, idx.long()] = val

                    def restore_dense():
                        dcol.copy_(col0)
                        dv.copy_(v0)

                    def run_dense():
                        ok(dense_warm(p(D), nr, nc, B, None, p(dcol), None, p(du), p(dv), p(dkept), TIE, stream))

                    variants["dense_warm_ms"] = (run_dense, restore_dense)
                out = {"nr": nr, "nc": nc, "B": B, "density": density, "nnz": nnz, "k": k}
                out.update(timed(variants))
                # what the last round left: the warm result (warm_ms runs after prologue_ms), the cold and dense ones
                restore()
                run_warm()
                out["kept_mean"] = float(kept.float().mean())
                cflags = santa_hip.check_duals_sparse(crow, idx, val, (B, nr, nc), col, u, v, validate=False)[1]
                out["certified"] = not bool(cflags.any())
                assert out["certified"], cflags.tolist()
                if dense:
                    out["equals_dense"] = bool(torch.equal(col, dcol) and torch.equal(kept, dkept))
                    assert out["equals_dense"]
                    del D
                if args.tag:
                    out["tag"] = args.tag
                line = json.dumps(out)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
