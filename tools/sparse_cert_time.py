"""dev: what the certificates on the CSR cost.
    python tools/sparse_cert_time.py [--out profiles/lsap_sparse_cert.jsonl] [--nc 1024,4096] [--part cert,match]
Method (tools/lbap_time.py's): device events around the whole C-ABI call on preallocated buffers, one
warm-up, then the median of 5, in ms; the two sides of a comparison alternate.  One JSON line per case.

part "cert": lsap_check_duals_csr_f64 against the only way there was, lsap_check_duals_large_f64 on the
  densification of the same instances (built on the device, not timed), on the (col, u, v) that
  lsap_solve_csr_f64 returns: square n x n instances, n in --nc, the diagonal plus a random pattern of 1 %,
  5 % and 40 %, values uniform in [0, 100); B = 64 at 1024 columns and 16 at 4096 (the dense batch is 2 GB).
  Both certificates must agree bit for bit.  bytes: 12 per stored entry against 8 per cell.
part "match": lsap_match_csr_f64 (both launches) against lsap_solve_csr_f64, the only feasibility test there
  was, on feasible random patterns (1 %, 5 %), on chain_open (row i holds {i, i + 1}, the last row {0}: the
  last search walks every row) and on a deficient pattern (1 % with 12 rows confined to 8 columns); the
  matching's card must equal the rows exactly where the solver finds an assignment.  scipy_ms: scipy's
  maximum_bipartite_matching over the same instances, one after the other on one CPU core (information)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-hungarian-method_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from santa_hip import _lib  # noqa: E402
from santa_hip.context import current_stream_handle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lsap_sparse_cert.jsonl"))
ap.add_argument("--nc", default="1024,4096")
ap.add_argument("--part", default="cert,match")
args = ap.parse_args()
assert torch.cuda.is_available(), "a measurement needs the GPU"
L = _lib.lib()
P = ctypes.c_void_p


def p(t):
    return P(t.data_ptr()) if t is not None and t.numel() else None


def timed_pair(a, b):
    """Median ms of a and of b over 5 alternating rounds after one warm-up each."""
    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    once(a), once(b)
    ta, tb = [], []
    for _ in range(5):
        ta.append(once(a))
        tb.append(once(b))
    return statistics.median(ta), statistics.median(tb)


def ok(rc):
    assert rc == 0, (rc, _lib.last_error())


def csr_of(Pm, seed):
    """(crow, idx, val) on the device of the pattern Pm bool [rows, n]."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    crow = torch.zeros(Pm.shape[0] + 1, dtype=torch.int64, device="cuda")
    crow[1:] = Pm.sum(1).cumsum(0)
    idx = Pm.nonzero()[:, 1].to(torch.int32).contiguous()
    val = torch.rand(idx.numel(), generator=g, device="cuda", dtype=torch.float64) * 100
    return crow, idx, val


def random_pattern(n, B, density, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Pm = torch.rand((B * n, n), generator=g, device="cuda") < density
    Pm[torch.arange(B * n, device="cuda"), torch.arange(n, device="cuda").repeat(B)] = True
    return Pm


def solve(crow, idx, val, n, B, work):
    col = torch.empty((B, n), dtype=torch.int32, device="cuda")
    u, v = torch.empty((B, n), dtype=torch.float64, device="cuda"), torch.empty((B, n), dtype=torch.float64, device="cuda")
    s = current_stream_handle(col.device)

    def call():
        ok(L.lsap_solve_csr_f64(p(crow), p(idx), p(val), n, n, B, None, p(col), None, p(u), p(v), p(work), work.numel(),
                                _lib.SH_COMPAT_TIEBREAK, s))
    return call, col, u, v


def batch_of(n):
    return 64 if n <= 1024 else 16


def part_cert(out):
    for n in (int(x) for x in args.nc.split(",")):
        B = batch_of(n)
        for density in (0.01, 0.05, 0.40):
            crow, idx, val = csr_of(random_pattern(n, B, density, 3), 4)
            work = torch.empty(int(L.lsap_csr_work_bytes(n, n, B)), dtype=torch.uint8, device="cuda")
            call, col, u, v = solve(crow, idx, val, n, B, work)
            call()
            torch.cuda.synchronize()
            assert bool((col >= 0).all())
            D = torch.full((B * n, n), float("inf"), dtype=torch.float64, device="cuda")
            D[torch.repeat_interleave(torch.arange(B * n, device="cuda"), crow[1:] - crow[:-1]), idx.long()] = val
            slack = [torch.empty((B, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
            flags = [torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2)]
            s = current_stream_handle(col.device)
            sparse_ms, dense_ms = timed_pair(
                lambda: ok(L.lsap_check_duals_csr_f64(p(crow), p(idx), p(val), n, n, B, None, p(col), p(u), p(v),
                                                      p(slack[0]), p(flags[0]), s)),
                lambda: ok(L.lsap_check_duals_large_f64(p(D), n, n, B, None, p(col), p(u), p(v), p(slack[1]),
                                                        p(flags[1]), s)))
            assert torch.equal(flags[0], flags[1]) and torch.equal(slack[0].view(torch.int64), slack[1].view(torch.int64))
            nnz = idx.numel()
            rec = {"part": "cert", "n": n, "B": B, "density": density, "nnz": nnz, "sparse_ms": sparse_ms,
                   "dense_ms": dense_ms, "sparse_over_dense": sparse_ms / dense_ms,
                   "sparse_bytes": 12 * nnz, "dense_bytes": 8 * B * n * n,
                   "sparse_gb_s": 12 * nnz / sparse_ms / 1e6, "dense_gb_s": 8 * B * n * n / dense_ms / 1e6,
                   "flagged": int((flags[0] != 0).sum())}
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            del D
            torch.cuda.empty_cache()


def patterns(n, B):
    yield "random_1pct", random_pattern(n, B, 0.01, 5)
    yield "random_5pct", random_pattern(n, B, 0.05, 5)
    chain = torch.zeros((n, n), dtype=torch.bool, device="cuda")
    i = torch.arange(n - 1, device="cuda")
    chain[i, i] = chain[i, i + 1] = True
    chain[n - 1, 0] = True
    yield "chain_open", chain.repeat(B, 1)
    Pm = random_pattern(n, B, 0.01, 6).view(B, n, n)
    g = torch.Generator(device="cuda").manual_seed(8)
    Pm[:, :12] = False
    Pm[:, :12, :8] = torch.rand((B, 12, 8), generator=g, device="cuda") < 0.6
    Pm[:, :12, 0] = True
    yield "deficient_12_on_8", Pm.view(B * n, n)


def part_match(out):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    for n in (int(x) for x in args.nc.split(",")):
        B = batch_of(n)
        for name, Pm in patterns(n, B):
            crow, idx, val = csr_of(Pm, 9)
            del Pm
            work = torch.empty(int(L.lsap_csr_work_bytes(n, n, B)), dtype=torch.uint8, device="cuda")
            solve_call, col, _, _ = solve(crow, idx, val, n, B, work)
            match = torch.empty((B, n), dtype=torch.int32, device="cuda")
            card = torch.empty(B, dtype=torch.int32, device="cuda")
            wit = torch.empty((B, n), dtype=torch.uint8, device="cuda")
            s = current_stream_handle(col.device)
            match_ms, solve_ms = timed_pair(
                lambda: ok(L.lsap_match_csr_f64(p(crow), p(idx), p(val), n, n, B, None, p(match), p(card), p(wit),
                                                p(work), work.numel(), 0, s)),
                solve_call)
            solved = (col >= 0).all(1)
            assert torch.equal(solved, card == n), name
            counts = torch.empty((B, 3), dtype=torch.int32, device="cuda")
            flags = torch.empty(B, dtype=torch.int32, device="cuda")
            ok(L.lsap_check_hall_csr_f64(p(crow), p(idx), p(val), n, n, B, None, p(match), p(wit), p(counts), p(flags), s))
            assert torch.equal(flags, torch.where(solved, 0, _lib.SH_HALL_DEFICIENT).to(torch.int32)), name
            hcrow, hidx = crow.cpu().numpy(), idx.cpu().numpy()
            t0 = time.perf_counter()
            cards = []
            for b in range(B):
                e0, e1 = hcrow[b * n], hcrow[(b + 1) * n]
                A = csr_matrix((np.ones(e1 - e0, dtype=np.int8), hidx[e0:e1], hcrow[b * n:(b + 1) * n + 1] - e0), shape=(n, n))
                cards.append(int((maximum_bipartite_matching(A, perm_type="column") >= 0).sum()))
            scipy_ms = (time.perf_counter() - t0) * 1e3
            assert cards == card.cpu().tolist(), name
            rec = {"part": "match", "pattern": name, "n": n, "B": B, "nnz": idx.numel(), "match_ms": match_ms,
                   "solve_ms": solve_ms, "match_over_solve": match_ms / solve_ms, "scipy_ms": scipy_ms,
                   "card_mean": float(card.float().mean()), "wit_rows_mean": float(wit.float().sum(1).mean())}
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            torch.cuda.empty_cache()


with open(args.out, "a") as out:
    if "cert" in args.part.split(","):
        part_cert(out)
    if "match" in args.part.split(","):
        part_match(out)
