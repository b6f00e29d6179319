"""Sparse (CSR) against dense batched LSAP on the same instances.

For n x n instances (default 2000 and 4096) at 1 %, 5 % and 25 % density and
batches of 16 and 256, times on the device
  * `sparse`  -- solve_batched_sparse (lsap_solve_csr_f64): the pass over the
                 CSR that fills the work buffer, then the solve;
  * `prep`    -- that first pass alone (SH_FLAG_BUILD_ONLY);
  * `dense`   -- solve_batched_large (lsap_solve_large_f64) on the
                 densification, +inf in the missing entries.
An instance is the diagonal (so it is feasible) plus uniform random entries,
values uniform integers in [0, 2^16) stored as float64, generated on the
device from a seed.  Both paths must return the same columns and the same cost
bits; a mismatch is counted in the record.

Timing: device events around the call, one warm-up and `--reps` timed runs of
each variant, alternating the variants inside a repetition; the record holds
the median and the spread (min, max).  Validation and the allocation of the
outputs and of the work buffer are inside the sparse and dense timings alike
(validate=False: the CSR is canonical by construction).

Prints one JSON object per line; a run is committed as profiles/lsap_sparse.jsonl.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-hungarian-method_amd"))

SEED = 7
MOD = 1 << 16


def make_batch(torch, B, n, density, dev):
    """(crow, col_indices, values, dense [B, n, n]) of B seeded instances."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED * 1000003 + n * 101 + int(density * 1000))
    D = torch.empty((B, n, n), dtype=torch.float64, device=dev)
    counts, idx, val = [], [], []
    eye = torch.eye(n, dtype=torch.bool, device=dev)
    for b in range(B):
        P = (torch.rand((n, n), generator=gen, device=dev) < density) | eye
        V = torch.randint(0, MOD, (n, n), generator=gen, device=dev).double()
        D[b] = torch.where(P, V, torch.full_like(V, float("inf")))
        counts.append(P.sum(dim=1))
        idx.append(P.nonzero()[:, 1].to(torch.int32))
        val.append(V[P])
    crow = torch.zeros(B * n + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.cat(counts), 0)
    return crow, torch.cat(idx), torch.cat(val), D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[2000, 4096])
    ap.add_argument("--density", type=float, nargs="*", default=[0.01, 0.05, 0.25])
    ap.add_argument("--batch", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the records to this file")
    a = ap.parse_args()

    import torch
    import santa_hip.lsap as L
    from santa_hip import _lib

    assert torch.cuda.is_available(), "sparse_sweep needs the MI355X"
    dev = torch.device("cuda", 0)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), res

    for n in a.n:
        for density in a.density:
            for B in a.batch:
                crow, idx, val, D = make_batch(torch, B, n, density, dev)
                shape = (B, n, n)
                variants = {
                    "sparse": lambda: L.solve_batched_sparse(crow, idx, val, shape=shape, validate=False),
                    "prep": lambda: L.solve_batched_sparse(crow, idx, val, shape=shape, validate=False,
                                                           flags=_lib.SH_FLAG_BUILD_ONLY),
                    "dense": lambda: L.solve_batched_large(D),
                }
                ms = {k: [] for k in variants}
                res = {}
                for k, fn in variants.items():  # warm-up (the results are compared below)
                    res[k] = once(fn)[1]
                for _ in range(a.reps):
                    for k, fn in variants.items():
                        ms[k].append(once(fn)[0])
                (scol, scost), (dcol, dcost) = res["sparse"], res["dense"]
                nnz = int(val.numel())
                rec = {"n": n, "density": density, "B": B, "nnz": nnz, "reps": a.reps,
                       "csr_bytes": nnz * 12 + (B * n + 1) * 8,
                       "work_bytes": int(_lib.lib().lsap_csr_work_bytes(n, n, B)),
                       "dense_bytes": B * n * n * 8,
                       "col_mismatches": int((scol != dcol).any(dim=1).sum()),
                       "cost_bit_mismatches": int((scost.view(torch.int64) != dcost.view(torch.int64)).sum()),
                       "infeasible": int((dcol < 0).any(dim=1).sum())}
                for k, t in ms.items():
                    rec[k + "_ms"] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3),
                                      "max": round(max(t), 3)}
                rec["sparse_over_dense"] = round(rec["sparse_ms"]["median"] / rec["dense_ms"]["median"], 3)
                emit(rec)
                del crow, idx, val, D, res
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
