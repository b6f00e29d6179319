"""GPU linear_sum_assignment — the inner seam of the reference.

`linear_sum_assignment(C)` is scipy's call at mpi_single.py:101 and
mpi_twins.py:104; this module mirrors its surface for any shape (the
reference produces square blocks; wide, tall and ragged batches are the
solver's own surface): same return value (row_ind, col_ind) as int64 numpy
arrays, same ValueError on NaN / -inf / infeasible input.  Solves run on the
GPU through the C-ABI batched solvers; float64 input is replayed with scipy's
own float64 arithmetic, so even the permutation on ties is scipy's.  Tall
input is solved as its transpose and inverted, as scipy does internally.
solve_batched also takes float32, float16 and bfloat16 device tensors: read at
their own width, widened in registers (exact) and solved as float64.
solve_batched(duals=True) and linear_sum_assignment_duals also return the dual
variables (u, v) the solve ends with, and check_duals certifies (col, u, v)
against the costs on the device: for integer costs flags == 0 proves optimality.
solve_batched_large, check_duals_large and linear_sum_assignment_large are the
same three up to SH_MAX_N_LARGE = 4096 rows or columns (the reference's own
block sizes, 2000 and 3000), through the lsap_*_large_ entries.
resolve_batched and linear_sum_assignment_resolve start from a previous
solution (col, v) of a nearby matrix instead of from nothing (the lsap_warm_
entries): one Dijkstra for each row whose pair did not survive.
solve_batched_sparse and linear_sum_assignment_sparse take the costs as CSR, a
missing entry being a forbidden pair (the lsap_solve_csr_ entries): the dense
float solve of the densification (densify), without the dense matrix.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .context import current_stream_handle, require_gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


INT64_COST_LIMIT = 1 << 50  # |C| bound that keeps every SAP value < 2^62 (n <= 1024)
INT64_COST_LIMIT_LARGE = 1 << 48  # the same factor 4n at n <= 4096
EXACT_INT_LIMIT = 1 << 53   # float64 holds every integer below this exactly
# floating-point cost dtypes of solve_batched and their C-ABI entries
FLOAT_ENTRIES = {torch.float64: "lsap_solve_batched_rect_f64", torch.float32: "lsap_solve_batched_rect_f32",
                 torch.float16: "lsap_solve_batched_rect_f16", torch.bfloat16: "lsap_solve_batched_rect_bf16"}
# every cost dtype -> the suffix of its lsap_solve_batched_duals_ / lsap_check_duals_ entry
DTYPE_SUFFIX = {torch.int64: "i64", torch.int32: "i32", torch.float64: "f64", torch.float32: "f32",
                torch.float16: "f16", torch.bfloat16: "bf16"}


# ---------------------------------------------------------------------------
# Host-only pieces (pure: no GPU, no library call).
# ---------------------------------------------------------------------------
def check_shapes(shapes, B: int, NR: int, NC: int) -> np.ndarray:
    """The per-instance shapes of a padded [B, NR, NC] batch as int32 [B, 2]
    on the host; ValueError unless 0 <= nr_b <= NR and nr_b <= nc_b <= NC."""
    if isinstance(shapes, torch.Tensor):
        shapes = shapes.detach().cpu().numpy()
    sh = np.asarray(shapes)
    if sh.shape != (B, 2) or not np.issubdtype(sh.dtype, np.integer):
        raise ValueError(f"shapes must be an integer [B, 2] = [{B}, 2] array, got {sh.dtype} {sh.shape}")
    sh = sh.astype(np.int64)
    nr, nc = sh[:, 0], sh[:, 1]
    bad = np.flatnonzero((nr < 0) | (nr > NR) | (nc < 0) | (nc > NC))
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"shapes[{b}] = ({int(nr[b])}, {int(nc[b])}) is outside the padded "
                         f"[{NR}, {NC}] matrix")
    tall = np.flatnonzero(nr > nc)
    if tall.size:
        b = int(tall[0])
        raise ValueError(f"shapes[{b}] = ({int(nr[b])}, {int(nc[b])}) is tall (nr > nc): "
                         "transpose the batch so that every instance has nr <= nc")
    return np.ascontiguousarray(sh, dtype=np.int32)


def invert_tall(col_t: torch.Tensor, nr: int) -> torch.Tensor:
    """col_t int32 [B, nc]: the solution of the transposed (wide) batch, i.e.
    the row of the tall matrix that each of its nc columns took (-1: none).
    Returns the tall batch's per-row columns, int32 [B, nr], -1 for the
    nr - nc rows left out (and everywhere for an infeasible instance)."""
    B, nc = col_t.shape
    out = torch.full((B, nr + 1), -1, dtype=torch.int32, device=col_t.device)
    idx = torch.where(col_t >= 0, col_t, torch.full_like(col_t, nr)).long()  # (-1 -> the spare slot)
    src = torch.arange(nc, dtype=torch.int32, device=col_t.device).expand(B, nc)
    out.scatter_(1, idx, src)
    return out[:, :nr].contiguous()


def invert_col(col: torch.Tensor, n: int):
    """col int32 [B, m] with entries in [0, n) or -1 -> (inv int32 [B, n], bad
    bool [B]): inv[b, col[b, i]] = i and -1 where no row points.  bad marks the
    instances whose col is no partial assignment (an entry outside [-1, n), or
    two rows on one column), whose inverse means nothing."""
    B, m = col.shape
    ok = (col >= 0) & (col < n)
    inv = torch.full((B, n + 1), -1, dtype=torch.int32, device=col.device)
    idx = torch.where(ok, col, torch.full_like(col, n)).long()  # (anything else -> the spare slot)
    src = torch.arange(m, dtype=torch.int32, device=col.device).expand(B, m)
    inv.scatter_(1, idx, src)
    inv = inv[:, :n].contiguous()
    bad = ((~ok) & (col != -1)).any(1) | ((inv >= 0).sum(1) != ok.sum(1))
    return inv, bad


_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1


def narrow_col(col: torch.Tensor) -> torch.Tensor:
    """col of any signed integer dtype (or uint8) as the int32 the certificate
    entries read.  A value outside int32 saturates to INT32_MAX or INT32_MIN,
    which no kernel takes for a column (they flag it and never index with it);
    wrapping it would turn 2**32 + 3 into column 3.  TypeError for any other
    dtype."""
    if col.dtype == torch.int32:
        return col
    if col.dtype == torch.int64:
        return col.clamp(_INT32_MIN, _INT32_MAX).to(torch.int32)
    if col.dtype in (torch.int16, torch.int8, torch.uint8):
        return col.to(torch.int32)
    raise TypeError(f"col must be an integer tensor, got {col.dtype}")


def tall_result(col_t):
    """scipy's (row_ind, col_ind) of a tall matrix from the solution col_t of
    its transpose: rows sorted ascending, each with its column."""
    col_t = np.asarray(col_t, dtype=np.int64)
    order = np.argsort(col_t)
    return col_t[order], order.astype(np.int64)


def int64_cost_limit(n: int) -> int:
    """The bound |C| < limit of int64 costs for instances of max(NR, NC) = n:
    every value the shortest-augmenting-path run forms stays below 2^62, a
    factor 4n above the costs."""
    return INT64_COST_LIMIT if n <= _lib.SH_MAX_N else INT64_COST_LIMIT_LARGE


def exact_int64_route(C: np.ndarray) -> bool:
    """Whether an integer matrix is solved in exact int64: scipy solves in
    float64, and the int64 solve makes scipy's decisions only while every
    value scipy forms is an integer below 2^53 (no float64 rounding).  Duals
    and path lengths stay within a few max(nr, nc) * max|C|, so
    4 (max(nr, nc) + 1) max|C| < 2^53 is a safe bound.  It is taken in Python
    ints before any negation (np.abs / -C wrap at INT64_MIN)."""
    if not np.issubdtype(C.dtype, np.integer):
        return False
    if C.size == 0:
        return True
    return 4 * (max(C.shape) + 1) * max(int(C.max()), -int(C.min())) < EXACT_INT_LIMIT


# ---------------------------------------------------------------------------
def _check_int64_range(C: torch.Tensor):
    """ValueError unless an int64 batch is within int64_cost_limit of its size."""
    limit = int64_cost_limit(max(C.shape[1:]))
    # (max / -min as Python ints: abs() wraps at INT64_MIN)
    if C.dtype == torch.int64 and C.numel() and max(int(C.max()), -int(C.min())) >= limit:
        raise ValueError(f"int64 costs must satisfy |C| < 2**{limit.bit_length() - 1}; pass float64 instead")


def _solve_wide(C: torch.Tensor, with_cost: bool, fl: int, shape_dev, duals: bool, large: bool):
    """C contiguous [B, nr, nc], 1 <= nr <= nc (the square C-ABI entries are
    the rect ones with nr == nc and no shapes) -> (col, cost, u, v), u and v
    None without duals.  The entry by (large, duals, dtype): lsap_solve_large_
    (u and v nullable), lsap_solve_batched_duals_ or lsap_solve_batched_rect_."""
    B, nr, nc = C.shape
    dev = C.device
    if C.dtype not in DTYPE_SUFFIX:
        raise TypeError(f"unsupported dtype {C.dtype}")
    _check_int64_range(C)
    ddt = torch.float64 if C.dtype in FLOAT_ENTRIES else torch.int64
    col = torch.empty((B, nr), dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=ddt, device=dev) if with_cost else None
    u = torch.empty((B, nr), dtype=ddt, device=dev) if duals else None
    v = torch.empty((B, nc), dtype=ddt, device=dev) if duals else None
    name = "lsap_solve_large" if large else "lsap_solve_batched_duals" if duals else "lsap_solve_batched_rect"
    uv = (_p(u), _p(v)) if large or duals else ()
    rc = getattr(_lib.lib(), f"{name}_{DTYPE_SUFFIX[C.dtype]}")(
        _p(C), nr, nc, B, _p(shape_dev), _p(col), _p(cost), *uv, fl, current_stream_handle(dev))
    _lib.check(rc, "lsap_solve_batched" if name.endswith("rect") else name)
    return col, cost, u, v


def solve_batched(C: torch.Tensor, with_cost: bool = True, flags: int = 0, shapes=None,
                  maximize: bool = False, duals: bool = False):
    """C: device tensor [B, NR, NC] (int64 / int32 / float64 / float32 /
    float16 / bfloat16) -> (col int32 [B, NR], cost [B]), or with duals=True
    (col, cost, u [B, NR], v [B, NC]).

    The duals are the ones the shortest-augmenting-path run ends with, int64
    for integer costs and float64 otherwise, in the units of C:
    u[i] + v[j] <= C[i, j] on the live corner with equality on the chosen
    entries, v <= 0 with v == 0 on a column no row took, sum(u) + sum(v) ==
    cost.  Integer duals satisfy this exactly; float duals are bit for bit
    scipy's own and feasible up to its rounding.  A tall batch swaps the roles
    (u <= 0, 0 on the rows left out); maximize returns the negated duals of
    the negated problem (u[i] + v[j] >= C[i, j], v >= 0).  Padding gets 0, an
    infeasible instance NaN in its live slots.

    Floating-point costs are read at their own width and solved in float64
    (the widening is exact, and scipy converts to float64 before it solves):
    col and cost (float64) are bit for bit those of C.double().  Any other
    dtype raises TypeError.
    col[b, i] is the column of row i, -1 for a row without one: the NR - NC
    rows scipy leaves out of a tall instance, every row of an infeasible
    instance (floating point with +inf only), and the padded rows of a ragged one.
    `shapes` ([B, 2] integers, host or device) makes the batch ragged:
    instance b is the top-left shapes[b] = (nr_b, nc_b) corner of its padded
    matrix, 0 <= nr_b <= NR, nr_b <= nc_b <= NC; the padding is never read.
    Tall batches (NR > NC) are solved as their transpose and inverted on the
    device.  maximize negates the matrix (and the cost back).  int64 costs
    must satisfy |C| < 2^50 over the whole padded tensor (checked on the
    device)."""
    return _solve_batched(C, with_cost, flags, shapes, maximize, duals, False)


def solve_batched_large(C: torch.Tensor, with_cost: bool = True, flags: int = 0, shapes=None,
                        maximize: bool = False, duals: bool = False):
    """solve_batched up to SH_MAX_N_LARGE = 4096 rows or columns, through the
    lsap_solve_large_ entries: the same arguments, results and semantics.  Up
    to SH_MAX_N it runs solve_batched's kernels and returns its bits.  int64
    costs of a batch with max(NR, NC) > 1024 must satisfy |C| < 2^48
    (int64_cost_limit); flags may not force the one-wave float kernel
    (SH_FLAG_F64_SW) above 1024 columns."""
    return _solve_batched(C, with_cost, flags, shapes, maximize, duals, True)


def _solve_batched(C, with_cost, flags, shapes, maximize, duals, large):
    """solve_batched (limit SH_MAX_N) and solve_batched_large (SH_MAX_N_LARGE)."""
    require_gpu()
    if C.dim() != 3:
        raise ValueError("expected [B, NR, NC]")
    B, NR, NC = C.shape
    limit = _lib.SH_MAX_N_LARGE if large else _lib.SH_MAX_N
    if max(NR, NC) > limit:
        raise ValueError(f"max(NR, NC) = {max(NR, NC)} > {limit}")
    if C.dtype not in (torch.int64, torch.int32) and C.dtype not in FLOAT_ENTRIES:
        raise TypeError(f"unsupported dtype {C.dtype}")
    dev = C.device
    shape_dev = None
    if shapes is not None:
        if NR > NC:
            raise ValueError(f"a ragged batch must be padded wide, got [{NR}, {NC}]: "
                             "transpose the batch so that every instance has nr <= nc")
        shape_dev = torch.from_numpy(check_shapes(shapes, B, NR, NC)).to(dev)
    if B == 0 or NR == 0 or NC == 0:
        cdt = torch.float64 if C.dtype in FLOAT_ENTRIES else torch.int64
        out = (torch.full((B, NR), -1, dtype=torch.int32, device=dev),
               torch.zeros(B, dtype=cdt, device=dev) if with_cost else None)
        if duals:
            out += (torch.zeros((B, NR), dtype=cdt, device=dev), torch.zeros((B, NC), dtype=cdt, device=dev))
        return out
    if maximize:  # (int32: -INT32_MIN wraps, so widen; the int64 bound covers int64)
        C = -(C.to(torch.int64) if C.dtype == torch.int32 else C)
    fl = _lib.SH_COMPAT_TIEBREAK | flags
    if NR > NC:  # the transposed solve's row duals belong to the columns
        col_t, cost, v, u = _solve_wide(C.transpose(1, 2).contiguous(), with_cost, fl, None, duals, large)
        col = invert_tall(col_t, NR)
    else:
        col, cost, u, v = _solve_wide(C.contiguous(), with_cost, fl, shape_dev, duals, large)
    if maximize and cost is not None:
        cost = -cost
    if not duals:
        return col, cost
    return (col, cost, -u, -v) if maximize else (col, cost, u, v)


def solve_hash(seed: int, modulus: int, n: int, B: int, device: int | str = 0, with_cost: bool = True,
               nr: int | None = None):
    """Solve B device-generated n x n matrices (sampler.hash_matrix on the host);
    with nr, the first nr rows of each (an nr x n instance, nr <= n)."""
    require_gpu()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    col = torch.empty((B, n if nr is None else nr), dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.int64, device=dev) if with_cost else None
    L = _lib.lib()
    s = current_stream_handle(dev)
    if nr is None:
        rc = L.lsap_solve_batched_hash(ctypes.c_uint64(seed), ctypes.c_int64(modulus), n, B,
                                       _p(col), _p(cost), _lib.SH_COMPAT_TIEBREAK, s)
    else:
        rc = L.lsap_solve_batched_rect_hash(ctypes.c_uint64(seed), ctypes.c_int64(modulus), nr, n, B,
                                            _p(col), _p(cost), _lib.SH_COMPAT_TIEBREAK, s)
    _lib.check(rc, "lsap_solve_batched_hash")
    return col, cost


def check_duals(C: torch.Tensor, col: torch.Tensor, u: torch.Tensor, v: torch.Tensor, shapes=None,
                maximize: bool = False):
    """Certify (col, u, v) -- as solve_batched(duals=True) returns them, for the
    same C, shapes and maximize -- in one pass over the costs on the device.

    Returns (slack_min [B], tight_max [B], gap [B], flags int32 [B]); the
    first three are int64 for integer costs, float64 otherwise:
      slack_min  min over the live corner of (C[i, j] - u[i]) - v[j]
      tight_max  max over the live rows of |(C[i, col[i]] - u[i]) - v[col[i]]|
      gap        (sum u + sum v) - sum C[i, col[i]]
      flags      SH_CERT_* bits (santa_hip.h); for integer costs 0 proves the
                 instance optimal.
    maximize certifies the negated problem (-C, -u, -v), so the same signs
    hold.  A tall batch is checked as its transpose (a contiguous copy) with
    the duals swapped and col inverted.  col may have any integer dtype
    (TypeError otherwise); an int64 entry outside int32 is no column and sets
    SH_CERT_COL."""
    return _check_duals(C, col, u, v, shapes, maximize, False)


def check_duals_large(C: torch.Tensor, col: torch.Tensor, u: torch.Tensor, v: torch.Tensor, shapes=None,
                      maximize: bool = False):
    """check_duals up to SH_MAX_N_LARGE = 4096 rows or columns, through the
    lsap_check_duals_large_ entries: the same arguments, results and meaning."""
    return _check_duals(C, col, u, v, shapes, maximize, True)


def _check_duals(C, col, u, v, shapes, maximize, large):
    """check_duals (limit SH_MAX_N) and check_duals_large (SH_MAX_N_LARGE)."""
    require_gpu()
    if C.dim() != 3:
        raise ValueError("expected [B, NR, NC]")
    B, NR, NC = C.shape
    limit = _lib.SH_MAX_N_LARGE if large else _lib.SH_MAX_N
    if max(NR, NC) > limit:
        raise ValueError(f"max(NR, NC) = {max(NR, NC)} > {limit}")
    if C.dtype not in DTYPE_SUFFIX:
        raise TypeError(f"unsupported dtype {C.dtype}")
    ddt = torch.float64 if C.dtype in FLOAT_ENTRIES else torch.int64
    if tuple(col.shape) != (B, NR) or tuple(u.shape) != (B, NR) or tuple(v.shape) != (B, NC):
        raise ValueError(f"expected col and u of shape [{B}, {NR}] and v of shape [{B}, {NC}]")
    if u.dtype != ddt or v.dtype != ddt:
        raise TypeError(f"the duals of {C.dtype} costs are {ddt}")
    col = narrow_col(col)
    dev = C.device
    shape_dev = None
    if shapes is not None:
        if NR > NC:
            raise ValueError(f"a ragged batch must be padded wide, got [{NR}, {NC}]: "
                             "transpose the batch so that every instance has nr <= nc")
        shape_dev = torch.from_numpy(check_shapes(shapes, B, NR, NC)).to(dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    slack = torch.zeros((B, 3), dtype=ddt, device=dev)
    if B == 0 or NR == 0 or NC == 0:
        return slack[:, 0], slack[:, 1], slack[:, 2], flags
    if maximize:
        C, u, v = -(C.to(torch.int64) if C.dtype == torch.int32 else C), -u, -v
    bad = None
    if NR > NC:
        C, u, v = C.transpose(1, 2), v, u
        col, bad = invert_col(col, NC)
        NR, NC = NC, NR
    C, col, u, v = C.contiguous(), col.contiguous(), u.contiguous(), v.contiguous()
    entry = getattr(_lib.lib(), ("lsap_check_duals_large_" if large else "lsap_check_duals_") + DTYPE_SUFFIX[C.dtype])
    rc = entry(_p(C), NR, NC, B, _p(shape_dev), _p(col), _p(u), _p(v), _p(slack), _p(flags),
               current_stream_handle(dev))
    _lib.check(rc, "lsap_check_duals")
    if bad is not None:  # a tall col that was no assignment before its inversion
        flags = flags | (bad.to(torch.int32) * _lib.SH_CERT_COL)
    return slack[:, 0], slack[:, 1], slack[:, 2], flags


def _route(cost_matrix, maximize: bool, dev, limit: int = _lib.SH_MAX_N):
    """linear_sum_assignment's host side: the wide device matrix to minimise
    (int64 on the exact route, float64 otherwise) and whether the input was
    tall; None for an empty matrix."""
    C = np.asarray(cost_matrix)
    if C.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %r array" % (C.shape,))
    nr, nc = C.shape
    if nr == 0 or nc == 0:
        return None, False
    if max(nr, nc) > limit:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {limit}")
    if C.dtype == np.bool_:
        C = C.astype(np.int64)
    if np.issubdtype(C.dtype, np.unsignedinteger):
        # negating an unsigned array wraps: widen first (uint64 beyond int64 -> float64)
        C = C.astype(np.int64) if (C.size == 0 or int(C.max()) <= np.iinfo(np.int64).max) \
            else C.astype(np.float64)
    tall = nr > nc
    if tall:  # scipy solves the transpose and re-orders the result (tall_result)
        C = C.T
    # Integer ranges wider than exact_int64_route allows take the float64
    # replay of scipy's own arithmetic.
    if exact_int64_route(C):
        Ci = np.ascontiguousarray(C, dtype=np.int64)
        Ct = torch.from_numpy(-Ci if maximize else Ci).to(dev)
    else:
        Cf = np.ascontiguousarray(C, dtype=np.float64)
        if maximize:
            Cf = -Cf
        if np.isnan(Cf).any() or np.isneginf(Cf).any():
            raise ValueError("matrix contains invalid numeric entries")
        Ct = torch.from_numpy(Cf).to(dev)
    return Ct, tall


def _lsa(cost_matrix, maximize, device, duals, solve, limit):
    """The front ends' body: `solve` is solve_batched or solve_batched_large
    (looked up by the caller at call time), `limit` its size limit."""
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    Ct, tall = _route(cost_matrix, maximize, dev, limit)
    if Ct is None:
        z = np.zeros(0, dtype=np.int64)
        if not duals:
            return z, z.copy()
        nr, nc = np.asarray(cost_matrix).shape
        return z, z.copy(), np.zeros(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64)
    if not duals:
        col, _ = solve(Ct.unsqueeze(0), with_cost=False)
    else:
        col, _, u, v = solve(Ct.unsqueeze(0), with_cost=False, duals=True)
    col = col[0].cpu().numpy().astype(np.int64)
    if (col < 0).any():
        raise ValueError("cost matrix is infeasible")
    res = tall_result(col) if tall else (np.arange(col.size, dtype=np.int64), col)
    if not duals:
        return res
    u, v = u[0].cpu().numpy(), v[0].cpu().numpy()
    if maximize:
        u, v = -u, -v
    return res + ((v, u) if tall else (u, v))


def linear_sum_assignment_duals(cost_matrix, maximize: bool = False, device: int | str = 0):
    """linear_sum_assignment that also returns the dual variables:
    (row_ind, col_ind, u [nr], v [nc]), u and v numpy arrays, int64 on the
    exact integer route and float64 on the float64 route (the routing is
    linear_sum_assignment's).  u[i] + v[j] <= C[i, j] with equality on the
    returned pairs (>= with maximize), in the sense of solve_batched."""
    return _lsa(cost_matrix, maximize, device, True, solve_batched, _lib.SH_MAX_N)


def linear_sum_assignment(cost_matrix, maximize: bool = False, device: int | str = 0):
    """scipy.optimize.linear_sum_assignment for one matrix, solved on the GPU.

    Any shape up to SH_MAX_N on the longer side: wide input returns
    (arange(nr), col), tall input the rows scipy keeps, sorted, with their
    columns.  Integer matrices whose sums stay below 2^53 are solved in exact
    int64 (where scipy's float64 arithmetic is exact too); anything else in
    float64 with scipy's operation order, so the permutation is scipy's
    either way."""
    return _lsa(cost_matrix, maximize, device, False, solve_batched, _lib.SH_MAX_N)


def linear_sum_assignment_large(cost_matrix, maximize: bool = False, device: int | str = 0,
                                duals: bool = False):
    """linear_sum_assignment (or, with duals=True, linear_sum_assignment_duals)
    for any shape up to SH_MAX_N_LARGE = 4096 on the longer side: the same
    routing, results and errors, solved by solve_batched_large."""
    return _lsa(cost_matrix, maximize, device, duals, solve_batched_large, _lib.SH_MAX_N_LARGE)


# ---------------------------------------------------------------------------
# Warm start: re-solve from a previous assignment and its duals (the lsap_warm_
# entries).  The previous state is data: whatever it holds, the result is an
# optimal assignment with certified duals; the closer it is to optimal for the
# new costs, the fewer Dijkstras run (nr - kept of them).
# ---------------------------------------------------------------------------
def _check_resolve_args(C, col, u, v, shapes):
    """resolve_batched's host checks -> (B, NR, NC, duals dtype)."""
    if C.dim() != 3:
        raise ValueError("expected [B, NR, NC]")
    B, NR, NC = C.shape
    if max(NR, NC) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(NR, NC) = {max(NR, NC)} > {_lib.SH_MAX_N_LARGE}")
    if C.dtype not in DTYPE_SUFFIX:
        raise TypeError(f"unsupported dtype {C.dtype}")
    ddt = torch.float64 if C.dtype in FLOAT_ENTRIES else torch.int64
    if tuple(col.shape) != (B, NR) or tuple(u.shape) != (B, NR) or tuple(v.shape) != (B, NC):
        raise ValueError(f"expected col and u of shape [{B}, {NR}] and v of shape [{B}, {NC}]")
    if u.dtype != ddt or v.dtype != ddt:
        raise TypeError(f"the duals of {C.dtype} costs are {ddt}")
    narrow_col(col[:0])  # (TypeError unless an integer dtype)
    if shapes is not None and NR > NC:
        raise ValueError(f"a ragged batch must be padded wide, got [{NR}, {NC}]: "
                         "transpose the batch so that every instance has nr <= nc")
    return B, NR, NC, ddt


def resolve_batched(C: torch.Tensor, col: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                    with_cost: bool = True, flags: int = 0, shapes=None, maximize: bool = False):
    """solve_batched_large(duals=True) started from a previous solution
    (col [B, NR] of any integer dtype, u [B, NR], v [B, NC] with the duals'
    dtype) -> (col, cost, u, v, kept int32 [B]).

    C, shapes, maximize, the outputs' layout, padding and infeasibility are
    solve_batched_large's.  The previous solution is read as data and is not
    modified; it may belong to other costs, or be garbage: a column dual outside
    the window ([-2^56, 0] for integers, finite and <= 0 for floats, in the
    minimised problem) counts as 0, an entry of col outside [0, nc) as -1, and
    of two rows on one column the lower keeps it.  Of the two duals only the
    columns' are read (the rows' of a tall batch, which is solved as its
    transpose); the others are recomputed.  A tall instance whose col is no
    partial assignment (invert_col) starts from the empty matching.

    kept[b] pairs of the previous assignment survive and nr_b - kept[b]
    Dijkstras run.  The result is an optimal assignment with the signs and
    equalities check_duals_large tests (integer duals exact); among several
    optimal assignments it need not be the one solve_batched_large returns.
    flags: SH_FLAG_EXACT_ARGMIN; SH_FLAG_BUILD_ONLY returns the start state
    itself (the kept pairs, u, v, kept; cost 0)."""
    B, NR, NC, ddt = _check_resolve_args(C, col, u, v, shapes)
    shape_host = check_shapes(shapes, B, NR, NC) if shapes is not None else None
    require_gpu()
    dev = C.device
    if B == 0 or NR == 0 or NC == 0:
        return (torch.full((B, NR), -1, dtype=torch.int32, device=dev),
                torch.zeros(B, dtype=ddt, device=dev) if with_cost else None,
                torch.zeros((B, NR), dtype=ddt, device=dev), torch.zeros((B, NC), dtype=ddt, device=dev),
                torch.zeros(B, dtype=torch.int32, device=dev))
    col0 = narrow_col(col)
    if maximize:
        C, u, v = -(C.to(torch.int64) if C.dtype == torch.int32 else C), -u, -v
    tall = NR > NC
    if tall:  # the transpose: the rows' duals are its columns', col its inverse
        C, v0 = C.transpose(1, 2), u
        col0, bad = invert_col(col0, NC)
        col0[bad] = -1
        nr, nc = NC, NR
    else:
        v0, nr, nc = v, NR, NC
    C = C.contiguous()
    _check_int64_range(C)
    col_w = col0.clone().contiguous()
    v_w = v0.clone().contiguous()
    u_w = torch.empty((B, nr), dtype=ddt, device=dev)
    build_only = bool(flags & _lib.SH_FLAG_BUILD_ONLY)
    cost = (torch.zeros if build_only else torch.empty)(B, dtype=ddt, device=dev) if with_cost else None
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    shape_dev = torch.from_numpy(shape_host).to(dev) if shape_host is not None else None
    rc = getattr(_lib.lib(), "lsap_warm_" + DTYPE_SUFFIX[C.dtype])(
        _p(C), nr, nc, B, _p(shape_dev), _p(col_w), _p(cost), _p(u_w), _p(v_w), _p(kept),
        _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_warm")
    if tall:
        col_w, u_w, v_w = invert_tall(col_w, NR), v_w, u_w
    if maximize:
        cost = -cost if cost is not None else None
        u_w, v_w = -u_w, -v_w
    return col_w, cost, u_w, v_w, kept


def linear_sum_assignment_resolve(cost_matrix, col_ind, u, v, maximize: bool = False, device: int | str = 0):
    """linear_sum_assignment_large(duals=True) started from a previous solution
    of a nearby matrix -> (row_ind, col_ind, u, v).

    col_ind [nr] holds the previous column of every row, -1 for a row without
    one (for wide and square input that is the col_ind of an earlier call; from
    a tall result (r, c): full(nr, -1) with col_ind[r] = c); u [nr] and v [nc]
    are numpy arrays of the route's dtype, int64 on the exact integer route and
    float64 otherwise (linear_sum_assignment's routing; TypeError for another
    dtype).  The result is optimal; on ties it need not be scipy's permutation."""
    Ct, tall = _route(cost_matrix, maximize, torch.device("cpu"), _lib.SH_MAX_N_LARGE)
    nr, nc = np.asarray(cost_matrix).shape
    col_ind, u, v = np.asarray(col_ind), np.asarray(u), np.asarray(v)
    if col_ind.shape != (nr,) or u.shape != (nr,) or v.shape != (nc,):
        raise ValueError(f"expected col_ind and u of shape ({nr},) and v of shape ({nc},)")
    if not np.issubdtype(col_ind.dtype, np.integer):
        raise TypeError(f"col_ind must be an integer array, got {col_ind.dtype}")
    if Ct is None:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), np.zeros(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64)
    want = np.int64 if Ct.dtype == torch.int64 else np.float64
    if u.dtype != want or v.dtype != want:
        raise TypeError(f"this matrix is solved in {np.dtype(want).name}: u and v must have that dtype, "
                        f"got {u.dtype} and {v.dtype}")
    require_gpu()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    col0 = torch.from_numpy(np.clip(col_ind.astype(np.int64), _INT32_MIN, _INT32_MAX).astype(np.int32))[None]
    v0 = torch.from_numpy(np.ascontiguousarray(u if tall else v))[None]
    if maximize:
        v0 = -v0
    if tall:
        col0, bad = invert_col(col0, nc)
        col0[bad] = -1
    m = Ct.shape[0]
    col, _, ru, rv, _ = resolve_batched(Ct.unsqueeze(0).to(dev), col0.to(dev), torch.zeros((1, m), dtype=v0.dtype, device=dev),
                                        v0.to(dev), with_cost=False)
    col = col[0].cpu().numpy().astype(np.int64)
    if (col < 0).any():
        raise ValueError("cost matrix is infeasible")
    res = tall_result(col) if tall else (np.arange(col.size, dtype=np.int64), col)
    ru, rv = ru[0].cpu().numpy(), rv[0].cpu().numpy()
    if maximize:
        ru, rv = -ru, -rv
    return res + ((rv, ru) if tall else (ru, rv))


# ---------------------------------------------------------------------------
# Sparse (CSR) costs: a missing entry is a forbidden pair.  A sparse instance
# is solved exactly as the dense float solver solves its densification.
# ---------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def densify(crow, col_indices, values, shape) -> np.ndarray:
    """The definition of a sparse instance (host-only): the float64 array of
    `shape` -- (B, NR, NC) for a batch stored as one CSR matrix of B * NR rows,
    or (nr, nc) for one matrix -- that holds each stored value (widened) and
    +inf everywhere else."""
    crow, idx = _np(crow).astype(np.int64), _np(col_indices).astype(np.int64)
    val = _np(values.double() if isinstance(values, torch.Tensor) else values)  # (bfloat16 has no numpy dtype)
    shape = tuple(int(s) for s in shape)
    rows = int(np.prod(shape[:-1]))
    if crow.size != rows + 1:
        raise ValueError(f"crow has {crow.size} entries, expected {rows + 1}")
    D = np.full((rows, shape[-1]), np.inf, dtype=np.float64)
    D[np.repeat(np.arange(rows), np.diff(crow)), idx] = val.astype(np.float64)
    return D.reshape(shape)


def csr_transpose(indptr, indices, data, shape):
    """(indptr, indices, data, (nc, nr)) of the transpose of an nr x nc CSR
    matrix, in pure numpy.  The sort by column is stable, so the entries of a
    new row keep the order of their old rows: canonical input gives canonical
    output."""
    indptr, indices, data = np.asarray(indptr, dtype=np.int64), np.asarray(indices), np.asarray(data)
    nr, nc = shape
    rows = np.repeat(np.arange(nr, dtype=indices.dtype if indices.size else np.int32), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    indptr_t = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=nc), out=indptr_t[1:])
    return indptr_t, rows[order], data[order], (nc, nr)


def validate_csr(crow, col_indices, values, shape, shapes=None) -> None:
    """ValueError unless (crow, col_indices, values) is the canonical CSR batch
    of `shape` = (B, NR, NC): crow[0] == 0, crow non-decreasing, crow[-1] ==
    nnz, indices in [0, NC) and strictly increasing inside each row, no NaN or
    -inf value (with `shapes`, none inside the instances' corners: what lies
    outside is never used).  Torch ops on the tensors' own device."""
    B, NR, NC = shape
    rows, nnz = B * NR, col_indices.numel()
    if crow.dim() != 1 or crow.numel() != rows + 1:
        raise ValueError(f"crow must have B * NR + 1 = {rows + 1} entries, got {tuple(crow.shape)}")
    if col_indices.dim() != 1 or values.dim() != 1 or values.numel() != nnz:
        raise ValueError("col_indices and values must be 1-D and of equal length")
    crow = crow.long()
    if int(crow[0]) != 0:
        raise ValueError("crow[0] != 0")
    if bool((crow[1:] < crow[:-1]).any()):
        raise ValueError("crow is decreasing somewhere")
    if int(crow[-1]) != nnz:
        raise ValueError(f"crow[-1] = {int(crow[-1])} != nnz = {nnz}")
    if nnz == 0:
        return
    idx = col_indices.long()
    if bool(((idx < 0) | (idx >= NC)).any()):
        raise ValueError(f"a column index lies outside [0, {NC})")
    first = torch.zeros(nnz + 1, dtype=torch.bool, device=idx.device)
    first[crow] = True  # the entries that begin a row
    if bool(((idx[1:] <= idx[:-1]) & ~first[1:nnz]).any()):
        raise ValueError("the column indices of a row are not strictly increasing")
    if values.is_floating_point():
        bad = torch.isnan(values) | (values == float("-inf"))
        if shapes is not None and bool(bad.any()):
            row = torch.repeat_interleave(torch.arange(rows, device=idx.device), crow[1:] - crow[:-1])
            sh = torch.as_tensor(np.asarray(_np(shapes), dtype=np.int64), device=idx.device)
            b = torch.div(row, NR, rounding_mode="floor")
            bad &= (row - b * NR < sh[b, 0]) & (idx < sh[b, 1])
        if bool(bad.any()):
            raise ValueError("matrix contains invalid numeric entries")


def _csr_parts(crow, col_indices, values, shape):
    """The (crow, col_indices, values, (B, NR, NC)) a sparse call means: the
    triple as given, or those of one 2-D torch.sparse_csr tensor [B * NR, NC]."""
    if isinstance(crow, torch.Tensor) and crow.layout == torch.sparse_csr:
        A = crow
        if A.dim() != 2:
            raise ValueError("expected one 2-D sparse CSR tensor of shape [B * NR, NC]")
        if shape is None:
            shape = (1,) + tuple(A.shape)
        crow, col_indices, values = A.crow_indices(), A.col_indices(), A.values()
        if tuple(A.shape) != (shape[0] * shape[1], shape[2]):
            raise ValueError(f"a sparse tensor of shape {tuple(A.shape)} is no batch of shape {tuple(shape)}")
    if shape is None or len(shape) != 3:
        raise ValueError("shape = (B, NR, NC) is required")
    return crow, col_indices, values, tuple(int(s) for s in shape)


def solve_batched_sparse(crow, col_indices=None, values=None, shape=None, with_cost: bool = True,
                         flags: int = 0, shapes=None, maximize: bool = False, duals: bool = False,
                         validate: bool = True):
    """solve_batched_large on sparse costs, a missing entry being a forbidden
    pair: each instance is solved exactly as solve_batched_large solves its
    densification (densify: the stored values, +inf elsewhere), with the same
    col, the same bits in cost, u and v, and -1 / cost 0 / NaN duals for an
    instance without a perfect matching of its rows.

    The batch is one CSR matrix of B * NR rows over NC columns, instance b in
    rows b * NR ..: crow [B * NR + 1] (int64 or int32), col_indices [nnz]
    (strictly increasing inside a row), values [nnz], all on one device, with
    shape = (B, NR, NC); or one 2-D torch.sparse_csr tensor [B * NR, NC] in
    place of the triple.  float64 and float32 values are read at their own
    width; integer and 16-bit values are converted to float64, as scipy does.
    A stored 0.0 is an edge of weight zero, a stored +inf a missing entry.
    1 <= NR <= NC <= SH_MAX_N_LARGE (NR > NC raises ValueError: transpose).
    `shapes` makes the batch ragged as in solve_batched; entries outside an
    instance's corner are ignored.  validate=True checks the CSR (validate_csr)
    on its device first; without it a malformed matrix gives an unspecified
    result, but nothing outside the buffers is touched.  flags: SH_FLAG_F64_MW /
    SH_FLAG_F64_SW as in solve_batched_large; SH_FLAG_BUILD_ONLY runs the first
    pass over the CSR alone and leaves the outputs unwritten (phase timing)."""
    crow, col_indices, values, shape = _csr_parts(crow, col_indices, values, shape)
    B, NR, NC = shape
    if B < 0 or NR < 0 or NC < 0:
        raise ValueError(f"negative size in shape {shape}")
    if NR > NC:
        raise ValueError(f"a sparse batch must be wide, got [{NR}, {NC}]: transpose it so that NR <= NC")
    if NC > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(NR, NC) = {NC} > {_lib.SH_MAX_N_LARGE}")
    if values.is_complex():
        raise TypeError(f"unsupported dtype {values.dtype}")
    if values.dtype not in (torch.float64, torch.float32):
        values = values.to(torch.float64)
    shape_host = check_shapes(shapes, B, NR, NC) if shapes is not None else None
    if validate:
        validate_csr(crow, col_indices, values, shape, shape_host)
    elif crow.numel() != B * NR + 1 or col_indices.numel() != values.numel():
        raise ValueError("crow must have B * NR + 1 entries, col_indices and values equal lengths")
    require_gpu()
    dev = values.device
    if B == 0 or NR == 0:
        out = (torch.full((B, NR), -1, dtype=torch.int32, device=dev),
               torch.zeros(B, dtype=torch.float64, device=dev) if with_cost else None)
        if duals:
            out += (torch.zeros((B, NR), dtype=torch.float64, device=dev),
                    torch.zeros((B, NC), dtype=torch.float64, device=dev))
        return out
    crow = crow.to(torch.int64).contiguous()
    col_indices = col_indices.to(torch.int32).contiguous()
    values = (-values if maximize else values).contiguous()
    shape_dev = torch.from_numpy(shape_host).to(dev) if shape_host is not None else None
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(NR, NC, B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    col = torch.empty((B, NR), dtype=torch.int32, device=dev)
    cost = torch.empty(B, dtype=torch.float64, device=dev) if with_cost else None
    u = torch.empty((B, NR), dtype=torch.float64, device=dev) if duals else None
    v = torch.empty((B, NC), dtype=torch.float64, device=dev) if duals else None
    entry = getattr(L, "lsap_solve_csr_" + DTYPE_SUFFIX[values.dtype])
    nnz = values.numel()
    rc = entry(_p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, NR, NC, B,
               _p(shape_dev), _p(col), _p(cost), _p(u), _p(v), _p(work), nbytes,
               _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_solve_csr")
    if maximize:
        cost = -cost if cost is not None else None
        if duals:
            u, v = -u, -v
    return (col, cost, u, v) if duals else (col, cost)


def _csr_of(A):
    """(indptr, indices, data, (nr, nc)) in numpy of linear_sum_assignment_sparse's
    argument, canonical when it comes from scipy.sparse or torch."""
    if hasattr(A, "tocsr"):  # a scipy.sparse matrix or array
        A = A.tocsr().copy()
        A.sum_duplicates()  # (also sorts the indices; stored zeros stay)
        return A.indptr, A.indices, A.data, tuple(A.shape)
    if isinstance(A, torch.Tensor):
        if A.layout != torch.sparse_csr or A.dim() != 2:
            raise ValueError("expected a 2-D torch.sparse_csr tensor")
        val = A.values()
        if val.dtype in (torch.float16, torch.bfloat16):
            val = val.double()
        return _np(A.crow_indices()), _np(A.col_indices()), _np(val), tuple(A.shape)
    indptr, indices, data, shape = A
    return _np(indptr), _np(indices), _np(data), tuple(int(s) for s in shape)


def linear_sum_assignment_sparse(A, maximize: bool = False, device: int | str = 0, duals: bool = False):
    """linear_sum_assignment for one sparse matrix whose missing entries are
    forbidden pairs: (row_ind, col_ind) -- with duals=True also (u, v) -- of
    scipy's linear_sum_assignment on densify(A), ValueError("cost matrix is
    infeasible") where no full matching of the shorter side exists.

    A: a scipy.sparse matrix or array (anything with .tocsr()), a 2-D
    torch.sparse_csr tensor, or (indptr, indices, data, (nr, nc)).  Up to
    SH_MAX_N_LARGE on the longer side; tall input is transposed on the host
    (csr_transpose) and re-ordered as scipy does; empty input returns empty
    arrays."""
    indptr, indices, data, (nr, nc) = _csr_of(A)
    if nr == 0 or nc == 0:
        z = np.zeros(0, dtype=np.int64)
        return (z, z.copy(), np.zeros(nr), np.zeros(nc)) if duals else (z, z.copy())
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    if data.dtype not in (np.float64, np.float32):
        data = data.astype(np.float64)
    tall = nr > nc
    if tall:
        indptr, indices, data, (nr, nc) = csr_transpose(indptr, indices, data, (nr, nc))
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    out = solve_batched_sparse(torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
                               torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
                               torch.from_numpy(np.ascontiguousarray(data)).to(dev), shape=(1, nr, nc),
                               with_cost=False, maximize=maximize, duals=duals)
    col = out[0][0].cpu().numpy().astype(np.int64)
    if (col < 0).any():
        raise ValueError("cost matrix is infeasible")
    res = tall_result(col) if tall else (np.arange(col.size, dtype=np.int64), col)
    if not duals:
        return res
    u, v = out[2][0].cpu().numpy(), out[3][0].cpu().numpy()
    return res + ((v, u) if tall else (u, v))
