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
check_duals_sparse certifies such a solve on the CSR itself, and
maximum_matching_sparse, check_matching_sparse and maximum_bipartite_matching
find and prove a maximum-cardinality matching of the sparsity pattern: a
perfect matching of the rows, or a Hall violator where there is none (the
lsap_check_duals_csr_, lsap_match_csr_ and lsap_check_hall_csr_ entries).
resolve_batched_sparse and linear_sum_assignment_sparse_resolve are the warm
start on the CSR (the lsap_warm_csr_ entries): resolve_batched on the
densification, from a previous (col, v), without the dense matrix.
kbest_batched and kbest_assignments return the k best assignments (Murty's
partition on that warm start, pool and ranking on the device: the lsap_kbest_
entries); murty_children_batched is one expansion (lsap_murty_children_).
kbest_batched_sparse, kbest_assignments_sparse and murty_children_batched_sparse
are the same on the CSR (the lsap_kbest_csr_ and lsap_murty_children_csr_
entries): kbest_batched on the densification, without the dense matrix.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._batch import (_COL_DTYPES, DTYPE_SUFFIX, _INT32_MAX, _INT32_MIN, _p, alloc_outputs, check_solution, device_of,
                     empty_result, invert_col, minimised, narrow_col, plan, single_empty, single_result, tall_view,
                     wide_view)
from ._batch import check_shapes, invert_tall, tall_result  # noqa: F401  (re-exported: they lived here)
from .context import current_stream_handle, require_gpu

INT64_COST_LIMIT = 1 << 50  # |C| bound that keeps every SAP value < 2^62 (n <= 1024)
INT64_COST_LIMIT_LARGE = 1 << 48  # the same factor 4n at n <= 4096
EXACT_INT_LIMIT = 1 << 53   # float64 holds every integer below this exactly
# floating-point cost dtypes of solve_batched and their C-ABI entries
FLOAT_ENTRIES = {torch.float64: "lsap_solve_batched_rect_f64", torch.float32: "lsap_solve_batched_rect_f32",
                 torch.float16: "lsap_solve_batched_rect_f16", torch.bfloat16: "lsap_solve_batched_rect_bf16"}


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
    """solve_batched (limit SH_MAX_N) and solve_batched_large (SH_MAX_N_LARGE).
    The entry by (large, duals, dtype): lsap_solve_large_ (u and v nullable),
    lsap_solve_batched_duals_ or lsap_solve_batched_rect_ (the square C-ABI
    entries are the rect ones with nr == nc and no shapes)."""
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE if large else _lib.SH_MAX_N, shapes)
    dev = C.device
    if p.empty:
        return empty_result(p, with_cost, duals, p.ddt, dev)
    require_gpu()
    if maximize:
        C, = minimised(C)
    if p.tall:
        C, _, _ = wide_view(C)
    C = C.contiguous()
    _check_int64_range(C)
    col, cost, u, v = alloc_outputs(p, with_cost, duals, p.ddt, dev)
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    name = "lsap_solve_large" if large else "lsap_solve_batched_duals" if duals else "lsap_solve_batched_rect"
    uv = (_p(u), _p(v)) if large or duals else ()
    rc = getattr(_lib.lib(), f"{name}_{DTYPE_SUFFIX[C.dtype]}")(
        _p(C), p.nr, p.nc, p.B, _p(shape_dev), _p(col), _p(cost), *uv,
        _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_solve_batched" if name.endswith("rect") else name)
    if p.tall:
        col, u, v = tall_view(p, col, u, v)
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
    dev = device_of(device)
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
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE if large else _lib.SH_MAX_N, shapes)
    check_solution(p, C.dtype, col, u, v)
    dev = C.device
    flags = torch.zeros(p.B, dtype=torch.int32, device=dev)
    slack = torch.zeros((p.B, 3), dtype=p.ddt, device=dev)
    if p.empty:
        return slack[:, 0], slack[:, 1], slack[:, 2], flags
    require_gpu()
    col, bad = narrow_col(col), None
    if maximize:
        C, u, v = minimised(C, u, v)
    if p.tall:
        C, u, v = wide_view(C, u, v)
        col, bad = invert_col(col, p.NC)
    C, col, u, v = C.contiguous(), col.contiguous(), u.contiguous(), v.contiguous()
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    entry = getattr(_lib.lib(), ("lsap_check_duals_large_" if large else "lsap_check_duals_") + DTYPE_SUFFIX[C.dtype])
    rc = entry(_p(C), p.nr, p.nc, p.B, _p(shape_dev), _p(col), _p(u), _p(v), _p(slack), _p(flags),
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
    Ct, tall = _route(cost_matrix, maximize, device_of(device), limit)
    if Ct is None:
        return single_empty(*np.asarray(cost_matrix).shape, duals)
    if not duals:
        return single_result(solve(Ct.unsqueeze(0), with_cost=False)[0], tall)
    col, _, u, v = solve(Ct.unsqueeze(0), with_cost=False, duals=True)
    return single_result(col, tall, u, v, negate=maximize)


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
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE, shapes)
    check_solution(p, C.dtype, col, u, v)
    dev = C.device
    if p.empty:
        return empty_result(p, with_cost, True, p.ddt, dev) + (torch.zeros(p.B, dtype=torch.int32, device=dev),)
    require_gpu()
    col0 = narrow_col(col)
    if maximize:
        C, u, v = minimised(C, u, v)
    if p.tall:  # the transpose: the rows' duals are its columns', col its inverse
        C, u, v = wide_view(C, u, v)
        col0, bad = invert_col(col0, p.NC)
        col0[bad] = -1
    C = C.contiguous()
    _check_int64_range(C)
    # the C entry works in place on col and v: it gets copies, and only u and the cost are new
    col_w, v_w = col0.clone().contiguous(), v.clone().contiguous()
    u_w = torch.empty((p.B, p.nr), dtype=p.ddt, device=dev)
    build_only = bool(flags & _lib.SH_FLAG_BUILD_ONLY)
    cost = (torch.zeros if build_only else torch.empty)(p.B, dtype=p.ddt, device=dev) if with_cost else None
    kept = torch.empty(p.B, dtype=torch.int32, device=dev)
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    rc = getattr(_lib.lib(), "lsap_warm_" + DTYPE_SUFFIX[C.dtype])(
        _p(C), p.nr, p.nc, p.B, _p(shape_dev), _p(col_w), _p(cost), _p(u_w), _p(v_w), _p(kept),
        _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_warm")
    if p.tall:
        col_w, u_w, v_w = tall_view(p, col_w, u_w, v_w)
    if maximize:
        cost = -cost if cost is not None else None
        u_w, v_w = -u_w, -v_w
    return col_w, cost, u_w, v_w, kept


def resolve_batched_free_rows(C: torch.Tensor, col: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                              with_cost: bool = True, flags: int = 0, shapes=None, maximize: bool = False):
    """resolve_batched for wide instances (nr < nc), solved as the padded
    square problem whose nc - nr extra rows cost 0 everywhere (the lsap_warm_fr_
    entries) -> (col, cost, u, v, kept int32 [B], kept_free
    int32 [B], theta [B] of the duals' dtype).

    The extra rows are never stored.  A square state needs no raising of column
    duals: a previous pair that is no longer tight costs one Dijkstra and
    breaks no other pair, where resolve_batched on a wide instance raises the
    dual of every free and broken column to 0, which with generic costs breaks
    most of the assignment.  The price is one Dijkstra for every virtual row
    whose column the start state does not hold (nc_b - nr_b - kept_free of
    them; none from the result of solve_batched_large or of an integer
    resolve) and up to nc - nr steps more in each Dijkstra, which read no
    memory but are steps.

    When it pays (measured on the MI355X with random costs):
    when nearly every column holds a row (nc - nr a few percent of nc) and few
    rows changed.  One redrawn row: 8x to 10x over a cold solve at 250 x 256
    and 4.4x to 6.6x at 1900 x 2000, where resolve_batched is no faster than
    the cold solve.  It breaks even with the cold solve at about 1 % redrawn
    rows at 1900 x 2000 (1.4x to 1.8x at 10 % of 250 x 256) and loses beyond:
    0.2x at 10 % of 1900 x 2000, 0.05x to 0.5x with every row redrawn, below
    resolve_batched.  With fewer rows than half the columns (64 x 1024, 1000 x
    2000) it loses from the first redrawn row, 0.03x to 0.33x of
    resolve_batched, which has little to raise there: use that.

    Arguments, layout, padding, tall batches (solved as their transpose),
    maximize, infeasibility and the reading of the previous state are
    resolve_batched's.  (nr_b - kept) + (nc_b - nr_b - kept_free) Dijkstras
    run.  theta is the largest column dual of the padded problem's final state
    (the smallest under maximize).

    Integer costs, nr_b < nc_b: u and v are the normalised duals u + theta and
    v - theta, exact, with the signs and equalities check_duals_large tests on
    the unpadded C; they may go back into this function or into
    resolve_batched.  Float costs: u and v are the padded problem's duals bit
    for bit; a free column holds v == theta up to rounding and not 0, so they
    are the input of this function's next call and not of resolve_batched, and
    check_duals_large's sign test does not apply to them.  A square instance
    gets what resolve_batched returns.
    flags: SH_FLAG_EXACT_ARGMIN; SH_FLAG_BUILD_ONLY returns the start state (the
    kept real pairs, u, v without a shift, the counts, its theta; cost 0)."""
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE, shapes)
    check_solution(p, C.dtype, col, u, v)
    dev = C.device
    if p.empty:
        z = torch.zeros(p.B, dtype=torch.int32, device=dev)
        return empty_result(p, with_cost, True, p.ddt, dev) + (z, z.clone(), torch.zeros(p.B, dtype=p.ddt, device=dev))
    require_gpu()
    col0 = narrow_col(col)
    if maximize:
        C, u, v = minimised(C, u, v)
    if p.tall:
        C, u, v = wide_view(C, u, v)
        col0, bad = invert_col(col0, p.NC)
        col0[bad] = -1
    C = C.contiguous()
    _check_int64_range(C)
    col_w, v_w = col0.clone().contiguous(), v.clone().contiguous()
    u_w = torch.empty((p.B, p.nr), dtype=p.ddt, device=dev)
    build_only = bool(flags & _lib.SH_FLAG_BUILD_ONLY)
    cost = (torch.zeros if build_only else torch.empty)(p.B, dtype=p.ddt, device=dev) if with_cost else None
    kept = torch.empty((p.B, 2), dtype=torch.int32, device=dev)
    theta = torch.empty(p.B, dtype=p.ddt, device=dev)
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    rc = getattr(_lib.lib(), "lsap_warm_fr_" + DTYPE_SUFFIX[C.dtype])(
        _p(C), p.nr, p.nc, p.B, _p(shape_dev), _p(col_w), _p(cost), _p(u_w), _p(v_w), _p(kept), _p(theta),
        _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_warm_fr")
    if p.tall:
        col_w, u_w, v_w = tall_view(p, col_w, u_w, v_w)
    if maximize:
        cost = -cost if cost is not None else None
        u_w, v_w, theta = -u_w, -v_w, -theta
    return col_w, cost, u_w, v_w, kept[:, 0].contiguous(), kept[:, 1].contiguous(), theta


def linear_sum_assignment_resolve(cost_matrix, col_ind, u, v, maximize: bool = False, device: int | str = 0,
                                  free_rows: bool = False):
    """linear_sum_assignment_large(duals=True) started from a previous solution
    of a nearby matrix -> (row_ind, col_ind, u, v).

    free_rows=True solves a rectangular matrix as its padded square problem
    (resolve_batched_free_rows, whose duals it returns: normalised on the exact
    integer route, the padded problem's on the float64 route).

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
        return single_empty(nr, nc, True)
    want = np.int64 if Ct.dtype == torch.int64 else np.float64
    if u.dtype != want or v.dtype != want:
        raise TypeError(f"this matrix is solved in {np.dtype(want).name}: u and v must have that dtype, "
                        f"got {u.dtype} and {v.dtype}")
    require_gpu()
    dev = device_of(device)
    col0 = torch.from_numpy(np.clip(col_ind.astype(np.int64), _INT32_MIN, _INT32_MAX).astype(np.int32))[None]
    v0 = torch.from_numpy(np.ascontiguousarray(u if tall else v))[None]
    if maximize:
        v0 = -v0
    if tall:
        col0, bad = invert_col(col0, nc)
        col0[bad] = -1
    m = Ct.shape[0]
    resolve = resolve_batched_free_rows if free_rows else resolve_batched
    col, _, ru, rv = resolve(Ct.unsqueeze(0).to(dev), col0.to(dev), torch.zeros((1, m), dtype=v0.dtype, device=dev),
                             v0.to(dev), with_cost=False)[:4]
    return single_result(col, tall, ru, rv, negate=maximize)


# ---------------------------------------------------------------------------
# The k best assignments (Murty's partition in fixed row order, DESIGN.md §20;
# the lsap_murty_children_ and lsap_kbest_ entries).  Float costs only: a child
# is its parent's matrix with +inf in places, and the integer solvers have no
# forbidden value.
# ---------------------------------------------------------------------------
KBEST_DTYPES = (torch.float64, torch.float32)


def _kbest_dtype(C):
    if C.dtype not in KBEST_DTYPES:
        raise TypeError(f"k-best assignments take float64 or float32 costs, got {C.dtype}: a subproblem forbids "
                        "pairs with +inf, and the integer solvers have no forbidden value (convert with .double())")


def forbidden_words(nc: int) -> int:
    """The 64-bit words of a node's forbidden-column bitmap over nc columns."""
    return (nc + 63) // 64


def murty_children_batched(C: torch.Tensor, col: torch.Tensor, v: torch.Tensor, p: torch.Tensor,
                           forb: torch.Tensor, shapes=None, free_rows: bool = False):
    """Expand one Murty node per instance into its NR children (the
    lsap_murty_children_ entries) -> (col int32 [B, NR, NR], cost float64
    [B, NR], u [B, NR, NR], v [B, NR, NC], kept int32 [B, NR]).

    C [B, NR, NC], NR <= NC <= SH_MAX_N, float64 or float32; the node of
    instance b is col[b] (any integer dtype), v[b] (float64 [NC]), p[b] (integer;
    negative: no node) and forb[b] (int64 [ceil(NC / 64)]: bit j & 63 of word
    j >> 6 forbids column j in row p).  Child t, p <= t < nr_b, is what
    resolve_batched computes from (col, v) on the matrix with rows < t fixed to
    their columns, those columns closed to the rows below, and forb (if
    t == p) and col[t] closed to row t; its slot is [b, t].  A child that does
    not exist or is infeasible has col -1 and cost +inf.  The node is read as
    data and not modified.

    free_rows=True (the lsap_murty_children_fr_ entries) computes every child
    as resolve_batched_free_rows does, on the masked matrix padded square with
    rows that cost 0 and are closed to the columns of the rows < t: the same
    optimum, one Dijkstra a child on a wide instance where the default raises
    column duals and runs many (measured at 250 x 256: 1 against 53 to 58 for
    the root's children).  v then holds the padded
    problem's column duals (a free column has v == theta up to rounding, not 0)
    and kept the real pairs; such a v is a node for free_rows=True only."""
    _kbest_dtype(C)
    p_ = plan(C.shape, C.dtype, _lib.SH_MAX_N, shapes)
    if p_.tall:
        raise ValueError(f"a Murty expansion takes a wide or square batch, got [{p_.NR}, {p_.NC}]")
    B, NR, NC = p_.B, p_.NR, p_.NC
    W = forbidden_words(NC)
    if tuple(col.shape) != (B, NR) or tuple(v.shape) != (B, NC) or tuple(p.shape) != (B,) \
            or tuple(forb.shape) != (B, W):
        raise ValueError(f"expected col [{B}, {NR}], v [{B}, {NC}], p [{B}] and forb [{B}, {W}]")
    if v.dtype != torch.float64:
        raise TypeError(f"the duals of {C.dtype} costs are torch.float64")
    if forb.dtype != torch.int64:
        raise TypeError("forb holds its 64-bit words as torch.int64")
    for name, x in (("col", col), ("p", p)):
        if x.dtype not in _COL_DTYPES:
            raise TypeError(f"{name} must be an integer tensor, got {x.dtype}")
    dev = C.device
    if p_.empty:
        return (torch.full((B, NR, NR), -1, dtype=torch.int32, device=dev),
                torch.full((B, NR), float("inf"), dtype=torch.float64, device=dev),
                torch.zeros((B, NR, NR), dtype=torch.float64, device=dev),
                torch.zeros((B, NR, NC), dtype=torch.float64, device=dev),
                torch.zeros((B, NR), dtype=torch.int32, device=dev))
    require_gpu()
    C = C.contiguous()
    col0, v0, p0, f0 = narrow_col(col).contiguous(), v.contiguous(), narrow_col(p).contiguous(), forb.contiguous()
    ccol = torch.empty((B, NR, NR), dtype=torch.int32, device=dev)
    cost = torch.empty((B, NR), dtype=torch.float64, device=dev)
    cu = torch.empty((B, NR, NR), dtype=torch.float64, device=dev)
    cv = torch.empty((B, NR, NC), dtype=torch.float64, device=dev)
    kept = torch.empty((B, NR), dtype=torch.int32, device=dev)
    shape_dev = p_.shapes_on(dev) if p_.shapes is not None else None
    entry = ("lsap_murty_children_fr_" if free_rows else "lsap_murty_children_") + DTYPE_SUFFIX[C.dtype]
    rc = getattr(_lib.lib(), entry)(
        _p(C), NR, NC, B, _p(shape_dev), _p(col0), _p(v0), _p(p0), _p(f0), _p(ccol), _p(cost), _p(cu), _p(cv),
        _p(kept), _lib.SH_COMPAT_TIEBREAK, current_stream_handle(dev))
    _lib.check(rc, "lsap_murty_children")
    return ccol, cost, cu, cv, kept


def kbest_batched(C: torch.Tensor, k: int, shapes=None, maximize: bool = False, free_rows: bool = False):
    """The k best assignments of every instance (the lsap_kbest_ entries) ->
    (cols int32 [B, k, NR], costs float64 [B, k], count int32 [B]).

    C [B, NR, NC] float64 or float32 (TypeError for any other dtype: the
    integer solvers have no forbidden value), up to SH_MAX_N rows or columns;
    shapes, maximize and tall batches as in resolve_batched.  Rank 0 is
    solve_batched_large's assignment, bit for bit; costs[b] is non-decreasing
    (non-increasing under maximize), the assignments of an instance are
    distinct, and count[b] <= k of them exist: the ranks beyond have col -1 and
    cost +inf (-inf under maximize).  cols[b, r, i] is the column of row i, -1
    for the rows a tall instance leaves out.  One call launches 3 k - 1 kernels
    whatever the data, allocates its pool once and never synchronises.

    free_rows=True (the lsap_kbest_fr_ entries) expands every node with
    murty_children_batched(free_rows=True): the same launches and pool, the
    same costs rank by rank (equal bits where every sum is exact); among
    assignments of equal cost the order and the choice may differ.  Measured
    (MI355X): an assignment of a 250 x 256 instance costs 2.5x to
    2.85x less and a 60 x 64 one 1.6x to 2.8x less, which is what they cost at
    256 x 256 and 64 x 64; a square instance is the same work either way (0.98x
    to 1.03x).  Not measured with far fewer rows than columns, where
    resolve_batched_free_rows itself loses: leave it off there."""
    _kbest_dtype(C)
    if int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    k = int(k)
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N, shapes)
    dev = C.device
    if p.empty:
        return (torch.full((p.B, k, p.NR), -1, dtype=torch.int32, device=dev),
                torch.full((p.B, k), float("-inf") if maximize else float("inf"), dtype=torch.float64, device=dev),
                torch.zeros(p.B, dtype=torch.int32, device=dev))
    require_gpu()
    if maximize:
        C, = minimised(C)
    if p.tall:
        C, _, _ = wide_view(C)
    C = C.contiguous()
    L = _lib.lib()
    nbytes = int(L.lsap_kbest_work_bytes(p.nr, p.nc, p.B, k))
    if nbytes == 0:
        raise ValueError(f"k = {k} is too large for a [{p.B}, {p.nr}, {p.nc}] batch")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    cols = torch.empty((p.B, k, p.nr), dtype=torch.int32, device=dev)
    costs = torch.empty((p.B, k), dtype=torch.float64, device=dev)
    count = torch.empty(p.B, dtype=torch.int32, device=dev)
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    rc = getattr(L, ("lsap_kbest_fr_" if free_rows else "lsap_kbest_") + DTYPE_SUFFIX[C.dtype])(
        _p(C), p.nr, p.nc, p.B, _p(shape_dev), k, _p(cols), _p(costs), _p(count), _p(work), nbytes,
        _lib.SH_COMPAT_TIEBREAK, current_stream_handle(dev))
    _lib.check(rc, "lsap_kbest")
    if p.tall:
        cols = invert_tall(cols.view(p.B * k, p.nr), p.NR).view(p.B, k, p.NR)
    if maximize:
        costs = -costs
    return cols, costs, count


def kbest_assignments(cost_matrix, k: int, maximize: bool = False, device: int | str = 0,
                      free_rows: bool = False):
    """The k best assignments of one matrix -> (col_inds int64 [m, nr], costs
    float64 [m]), m <= k the number that exist, best first.  col_inds[r, i] is
    the column of row i in the rank-r assignment, -1 for a row a tall matrix
    leaves out.  The matrix is solved in float64 (float32 input at its own
    width); +inf forbids a pair (under maximize: -inf), NaN and -inf (under
    maximize: +inf) raise ValueError as in linear_sum_assignment.  free_rows:
    kbest_batched's."""
    C = np.asarray(cost_matrix)
    if C.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %r array" % (C.shape,))
    if int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    nr, nc = C.shape
    if nr == 0 or nc == 0:
        return np.zeros((0, nr), dtype=np.int64), np.zeros(0, dtype=np.float64)
    if max(nr, nc) > _lib.SH_MAX_N:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N}")
    if C.dtype != np.float32:
        C = C.astype(np.float64)
    bad = -np.inf if not maximize else np.inf
    if np.isnan(C).any() or (C == bad).any():
        raise ValueError("matrix contains invalid numeric entries")
    Ct = torch.from_numpy(np.ascontiguousarray(C)).to(device_of(device))
    cols, costs, count = kbest_batched(Ct.unsqueeze(0), k, maximize=maximize, free_rows=free_rows)
    m = int(count[0])
    return cols[0, :m].cpu().numpy().astype(np.int64), costs[0, :m].cpu().numpy()


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


def _sparse_batch(crow, col_indices, values, shape, shapes, validate, pattern=False, limit=_lib.SH_MAX_N_LARGE):
    """The argument checks of a sparse batched call, in solve_batched_sparse's
    order -> (crow, col_indices, values, (B, NR, NC), its Batch); values
    float64 or float32.  pattern: values may be None (every stored entry counts),
    and stays None.  limit: the entry's largest NC."""
    crow, col_indices, values, shape = _csr_parts(crow, col_indices, values, shape)
    B, NR, NC = shape
    if B < 0 or NR < 0 or NC < 0:
        raise ValueError(f"negative size in shape {shape}")
    if NR > NC:
        raise ValueError(f"a sparse batch must be wide, got [{NR}, {NC}]: transpose it so that NR <= NC")
    if values is None and pattern:
        p = plan(shape, torch.float64, _lib.SH_MAX_N_LARGE, shapes)
        if validate:
            validate_csr(crow, col_indices, torch.zeros(col_indices.numel(), dtype=torch.float32,
                                                        device=col_indices.device), shape, p.shapes)
        elif crow.numel() != B * NR + 1:
            raise ValueError("crow must have B * NR + 1 entries")
        return crow, col_indices, None, shape, p
    if values.is_complex():
        raise TypeError(f"unsupported dtype {values.dtype}")
    if values.dtype not in (torch.float64, torch.float32):
        values = values.to(torch.float64)
    p = plan(shape, values.dtype, limit, shapes)
    if validate:
        validate_csr(crow, col_indices, values, shape, p.shapes)
    elif crow.numel() != B * NR + 1 or col_indices.numel() != values.numel():
        raise ValueError("crow must have B * NR + 1 entries, col_indices and values equal lengths")
    return crow, col_indices, values, shape, p


def _sparse_operands(p, crow, col_indices, values, maximize):
    """What the CSR entries read, after require_gpu(): int64 crow, int32
    indices, the values of the problem to minimise (None stays None) and the
    shapes on the device (None: not ragged)."""
    crow = crow.to(torch.int64).contiguous()
    col_indices = col_indices.to(torch.int32).contiguous()
    if values is not None:
        values = (-values if maximize else values).contiguous()
    dev = values.device if values is not None else crow.device
    return crow, col_indices, values, (p.shapes_on(dev) if p.shapes is not None else None)


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
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate)
    B, NR, NC = shape
    dev = values.device
    if p.empty:
        return empty_result(p, with_cost, duals, torch.float64, dev)
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, maximize)
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(NR, NC, B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    col, cost, u, v = alloc_outputs(p, with_cost, duals, torch.float64, dev)
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


# ---------------------------------------------------------------------------
# Certificates on the CSR itself: nothing is densified.  An
# edge is a stored entry of the live corner whose value is not +inf.
# ---------------------------------------------------------------------------
def check_duals_sparse(crow, col_indices, values, shape, col, u, v, shapes=None, maximize: bool = False,
                       validate: bool = True):
    """Certify (col, u, v) -- as solve_batched_sparse(duals=True) returns them,
    for the same batch, shapes and maximize -- in one pass over the stored
    entries: (slack float64 [B, 3], flags int32 [B]), bit for bit the
    (slack_min, tight_max, gap) and flags of check_duals_large on the
    densification (densify), a missing entry having slack +inf.  One rule is
    added: a live u or v that is not finite makes slack[:, 0] NaN and sets
    SH_CERT_SLACK (unless the instance is SH_CERT_NONE).  maximize certifies the
    negated problem, as check_duals does.  col may have any integer dtype; u and
    v are float64.  The batch, `shapes` and `validate` are solve_batched_sparse's."""
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate)
    check_solution(p, values.dtype, col, u, v)
    dev = values.device
    flags = torch.zeros(p.B, dtype=torch.int32, device=dev)
    slack = torch.zeros((p.B, 3), dtype=torch.float64, device=dev)
    if p.empty:
        return slack, flags
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, maximize)
    if maximize:
        u, v = -u, -v
    col, u, v = narrow_col(col).contiguous(), u.contiguous(), v.contiguous()
    nnz = values.numel()
    rc = getattr(_lib.lib(), "lsap_check_duals_csr_" + DTYPE_SUFFIX[values.dtype])(
        _p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, p.NR, p.NC, p.B, _p(shape_dev),
        _p(col), _p(u), _p(v), _p(slack), _p(flags), current_stream_handle(dev))
    _lib.check(rc, "lsap_check_duals_csr")
    return slack, flags


def maximum_matching_sparse(crow, col_indices=None, values=None, shape=None, shapes=None, maximize: bool = False,
                            validate: bool = True, flags: int = 0):
    """A maximum-cardinality matching of every instance's edges, batched
    (scipy.sparse.csgraph.maximum_bipartite_matching's problem), with the proof
    of its size: (match int32 [B, NR], card int32 [B], wit uint8 [B, NR]).

    The batch is solve_batched_sparse's: the triple with shape = (B, NR, NC), or
    one 2-D torch.sparse_csr tensor.  An edge is a stored entry whose value is
    not +inf (with maximize: not -inf); values=None means pattern only, every
    stored entry an edge.  match[b, i] is the column of row i or -1 (-1 in
    padded rows), card[b] the number of matched rows, the maximum.  wit[b] is the
    canonical Hall violator: 1 on every live row that an alternating path
    reaches from an unmatched row, all 0 when card == nr_b.  card and wit do
    not depend on which maximum matching was found; match need only be valid.
    check_matching_sparse checks the three against the CSR.  It is independent
    of the cost solver: card == nr_b exactly when solve_batched_sparse finds an
    assignment.  flags is reserved (one launch configuration)."""
    crow, col_indices, values, shape = _csr_parts(crow, col_indices, values, shape)
    if values is not None and maximize:
        values = -values  # (before the validation: the forbidden value is +inf from here on)
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate, pattern=True)
    dev = crow.device
    match = torch.full((p.B, p.NR), -1, dtype=torch.int32, device=dev)
    card = torch.zeros(p.B, dtype=torch.int32, device=dev)
    wit = torch.zeros((p.B, p.NR), dtype=torch.uint8, device=dev)
    if p.empty:
        return match, card, wit
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, False)
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(p.NR, p.NC, p.B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    entry = getattr(L, "lsap_match_csr_" + (DTYPE_SUFFIX[values.dtype] if values is not None else "f64"))
    nnz = col_indices.numel()
    rc = entry(_p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, p.NR, p.NC, p.B,
               _p(shape_dev), _p(match), _p(card), _p(wit), _p(work), nbytes, flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_match_csr")
    return match, card, wit


def check_matching_sparse(crow, col_indices, values, shape, match, wit, shapes=None, maximize: bool = False):
    """Check (match, wit) -- as maximum_matching_sparse returns them for the same
    batch, shapes and maximize, or anything else: they are read as data --
    against the CSR: (counts int32 [B, 3], flags int32 [B]).

    counts = (nM, nR, nN): the live rows with match != -1, the live rows with
    wit != 0, and the live columns an edge joins to one of those rows.  flags:
    SH_HALL_MATCH (match is no matching of the edges), SH_HALL_WITNESS
    (nR - nN != nr_b - nM) and SH_HALL_DEFICIENT (nM < nr_b).  Any row set R
    bounds every matching by nr_b - (|R| - |N(R)|): flags == 0 proves a perfect
    matching of the rows and exhibits it, SH_HALL_DEFICIENT alone proves there
    is none and that nM is the maximum.  match [B, NR] may have any integer
    dtype, wit [B, NR] is uint8 or bool; values may be None (pattern only)."""
    if values is not None and maximize:
        values = -values
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, False, pattern=True)
    if tuple(match.shape) != (p.B, p.NR) or tuple(wit.shape) != (p.B, p.NR):
        raise ValueError(f"expected match and wit of shape [{p.B}, {p.NR}]")
    if wit.dtype not in (torch.uint8, torch.bool):
        raise TypeError("wit must be uint8 or bool")
    dev = crow.device
    counts = torch.zeros((p.B, 3), dtype=torch.int32, device=dev)
    flags = torch.zeros(p.B, dtype=torch.int32, device=dev)
    match = narrow_col(match)
    if p.empty:
        return counts, flags
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, False)
    match, wit = match.contiguous(), wit.to(torch.uint8).contiguous()
    entry = getattr(_lib.lib(), "lsap_check_hall_csr_" + (DTYPE_SUFFIX[values.dtype] if values is not None else "f64"))
    nnz = col_indices.numel()
    rc = entry(_p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, p.NR, p.NC, p.B,
               _p(shape_dev), _p(match), _p(wit), _p(counts), _p(flags), current_stream_handle(dev))
    _lib.check(rc, "lsap_check_hall_csr")
    return counts, flags


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
        return single_empty(nr, nc, duals, np.float64)
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    if data.dtype not in (np.float64, np.float32):
        data = data.astype(np.float64)
    tall = nr > nc
    if tall:
        indptr, indices, data, (nr, nc) = csr_transpose(indptr, indices, data, (nr, nc))
    dev = device_of(device)
    out = solve_batched_sparse(torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
                               torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
                               torch.from_numpy(np.ascontiguousarray(data)).to(dev), shape=(1, nr, nc),
                               with_cost=False, maximize=maximize, duals=duals)
    return single_result(out[0], tall, *out[2:])  # (the duals come back in the matrix's own signs)


# ---------------------------------------------------------------------------
# Warm start on the CSR (the lsap_warm_csr_ entries):
# resolve_batched on the densification, without the dense matrix.
# ---------------------------------------------------------------------------
def resolve_batched_sparse(crow, col_indices, values, shape, col, u, v, with_cost: bool = True, flags: int = 0,
                           shapes=None, maximize: bool = False, validate: bool = True):
    """solve_batched_sparse(duals=True) started from a previous solution (col
    [B, NR] of any integer dtype, u [B, NR], v [B, NC] float64) -> (col, cost,
    u, v, kept int32 [B]): what resolve_batched returns for the densification
    (densify) with the same shapes and the same previous col and v -- the same
    col and kept, the same bits in cost, u and v equal by value (a zero may
    carry the other sign) -- without building it.

    The batch, `shapes`, `validate` and maximize are solve_batched_sparse's (the
    triple with shape = (B, NR, NC), or one 2-D torch.sparse_csr tensor in place
    of crow); the previous solution is resolve_batched's: read as data, not
    modified, of any content, and of the two duals only v is read.  The pattern
    may have changed as well as the values: a previous pair that is no longer
    stored is dropped, a new entry is an edge.  An instance without a perfect
    matching of its rows gets -1, cost 0 and NaN duals.  flags:
    SH_FLAG_BUILD_ONLY returns the start state itself (the kept pairs, u, v,
    kept; cost 0), as on resolve_batched."""
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate)
    check_solution(p, values.dtype, col, u, v)
    dev = values.device
    if p.empty:
        return empty_result(p, with_cost, True, p.ddt, dev) + (torch.zeros(p.B, dtype=torch.int32, device=dev),)
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, maximize)
    # the C entry works in place on col and v: it gets copies, and only u and the cost are new
    col_w = narrow_col(col).clone().contiguous()
    v_w = (-v if maximize else v.clone()).contiguous()
    u_w = torch.empty((p.B, p.NR), dtype=torch.float64, device=dev)
    build_only = bool(flags & _lib.SH_FLAG_BUILD_ONLY)
    cost = (torch.zeros if build_only else torch.empty)(p.B, dtype=torch.float64, device=dev) if with_cost else None
    kept = torch.empty(p.B, dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(p.NR, p.NC, p.B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nnz = values.numel()
    rc = getattr(L, "lsap_warm_csr_" + DTYPE_SUFFIX[values.dtype])(
        _p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, p.NR, p.NC, p.B, _p(shape_dev),
        _p(col_w), _p(cost), _p(u_w), _p(v_w), _p(kept), _p(work), nbytes, _lib.SH_COMPAT_TIEBREAK | flags,
        current_stream_handle(dev))
    _lib.check(rc, "lsap_warm_csr")
    if maximize:
        cost = -cost if cost is not None else None
        u_w, v_w = -u_w, -v_w
    return col_w, cost, u_w, v_w, kept


def resolve_batched_sparse_free_rows(crow, col_indices, values, shape, col, u, v, with_cost: bool = True,
                                     flags: int = 0, shapes=None, maximize: bool = False, validate: bool = True):
    """resolve_batched_sparse for wide instances (nr < nc), solved as the padded
    square problem whose nc - nr extra rows cost 0 everywhere (the
    lsap_warm_fr_csr_ entries) -> (col, cost, u, v, kept int32
    [B], kept_free int32 [B], theta float64 [B]): what resolve_batched_free_rows
    returns for the densification (densify) with the same shapes and the same
    previous col and v -- the same col, kept and kept_free, the same bits in
    cost, u, v and theta equal by value (a zero may carry the other sign) --
    without building it.

    The extra rows are never stored and read no entry of the CSR; they cannot
    make an instance infeasible, and an instance without a perfect matching of
    its real rows gets -1, cost 0, NaN duals and NaN theta.  The batch,
    `shapes`, `validate`, maximize and the reading of the previous state are
    resolve_batched_sparse's: a previous pair that is no longer stored is
    dropped, a new entry is an edge.  (nr_b - kept) + (nc_b - nr_b - kept_free)
    Dijkstras run.  u and v are the padded problem's duals as the solver left
    them (no shift): a free column holds v == theta up to rounding and not 0, so
    they are the input of this function's next call and not of
    resolve_batched_sparse.  A square instance gets what resolve_batched_sparse
    returns.  flags: SH_FLAG_BUILD_ONLY returns the start state (the kept real
    pairs, u, v, both counts, its theta; cost 0).

    When it pays (measured on the MI355X, 64 instances, band patterns at 1 %,
    5 % and 40 % density): when nearly every column holds a row
    and few rows changed.  One redrawn row re-solves 5.4x to 9.3x faster than
    resolve_batched_sparse at 250 x 256, 12x to 20x at 1018 x 1024 and 5.0x to
    6.5x at 1900 x 2000 (about the same over a cold solve_batched_sparse, which
    resolve_batched_sparse does not beat there); 1 % of the rows: 3.8x to 6.7x,
    4.5x to 4.8x and 1.1x to 1.3x; 10 %: 1.2x to 1.5x up to 1024 columns, but
    0.2x to 0.3x at 1900 x 2000; with every row redrawn it loses everywhere
    (0.55x to 0.8x up to 1024 columns, 0.08x to 0.11x at 2000), and an
    unchanged batch costs 2 % to 6 % more than resolve_batched_sparse.  With
    few rows on many columns (64 x 1024) it loses from the first row, 0.02x to
    0.45x of resolve_batched_sparse: use that.  Against
    resolve_batched_free_rows on a densification built beforehand it takes
    0.94x to 1.15x the time at 1 % density and 1.0x to 1.7x at 5 % and 40 % once
    a row changed.
    """
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate)
    check_solution(p, values.dtype, col, u, v)
    dev = values.device
    if p.empty:
        z = torch.zeros(p.B, dtype=torch.int32, device=dev)
        return empty_result(p, with_cost, True, p.ddt, dev) + (z, z.clone(),
                                                               torch.zeros(p.B, dtype=torch.float64, device=dev))
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, maximize)
    # the C entry works in place on col and v: it gets copies, and only u and the cost are new
    col_w = narrow_col(col).clone().contiguous()
    v_w = (-v if maximize else v.clone()).contiguous()
    u_w = torch.empty((p.B, p.NR), dtype=torch.float64, device=dev)
    build_only = bool(flags & _lib.SH_FLAG_BUILD_ONLY)
    cost = (torch.zeros if build_only else torch.empty)(p.B, dtype=torch.float64, device=dev) if with_cost else None
    kept = torch.empty((p.B, 2), dtype=torch.int32, device=dev)
    theta = torch.empty(p.B, dtype=torch.float64, device=dev)
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(p.NR, p.NC, p.B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nnz = values.numel()
    rc = getattr(L, "lsap_warm_fr_csr_" + DTYPE_SUFFIX[values.dtype])(
        _p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, p.NR, p.NC, p.B, _p(shape_dev),
        _p(col_w), _p(cost), _p(u_w), _p(v_w), _p(kept), _p(theta), _p(work), nbytes,
        _lib.SH_COMPAT_TIEBREAK | flags, current_stream_handle(dev))
    _lib.check(rc, "lsap_warm_fr_csr")
    if maximize:
        cost = -cost if cost is not None else None
        u_w, v_w, theta = -u_w, -v_w, -theta
    return col_w, cost, u_w, v_w, kept[:, 0].contiguous(), kept[:, 1].contiguous(), theta


def linear_sum_assignment_sparse_resolve(A, col_ind, u, v, maximize: bool = False, device: int | str = 0,
                                         free_rows: bool = False):
    """linear_sum_assignment_sparse(duals=True) started from a previous solution
    of a nearby matrix -> (row_ind, col_ind, u, v).

    free_rows=True solves a rectangular matrix as its padded square problem
    (resolve_batched_sparse_free_rows, whose duals it returns: the padded
    problem's, the input of the next call with free_rows=True).

    A is linear_sum_assignment_sparse's; col_ind [nr], u [nr] and v [nc] are
    linear_sum_assignment_resolve's, the duals float64 numpy arrays (TypeError
    otherwise).  Tall input is solved as its transpose (csr_transpose) from the
    inverse of col_ind and from u.  The result is optimal; on ties it need not
    be scipy's permutation.  ValueError("cost matrix is infeasible") where no
    full matching of the shorter side exists."""
    indptr, indices, data, (nr, nc) = _csr_of(A)
    col_ind, u, v = np.asarray(col_ind), np.asarray(u), np.asarray(v)
    if col_ind.shape != (nr,) or u.shape != (nr,) or v.shape != (nc,):
        raise ValueError(f"expected col_ind and u of shape ({nr},) and v of shape ({nc},)")
    if not np.issubdtype(col_ind.dtype, np.integer):
        raise TypeError(f"col_ind must be an integer array, got {col_ind.dtype}")
    if nr == 0 or nc == 0:
        return single_empty(nr, nc, True, np.float64)
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    if u.dtype != np.float64 or v.dtype != np.float64:
        raise TypeError(f"a sparse matrix is solved in float64: u and v must have that dtype, "
                        f"got {u.dtype} and {v.dtype}")
    if data.dtype not in (np.float64, np.float32):
        data = data.astype(np.float64)
    require_gpu()
    dev = device_of(device)
    col0 = torch.from_numpy(np.clip(col_ind.astype(np.int64), _INT32_MIN, _INT32_MAX).astype(np.int32))[None]
    tall = nr > nc
    v0 = torch.from_numpy(np.ascontiguousarray(u if tall else v))[None]
    if tall:
        indptr, indices, data, (nr, nc) = csr_transpose(indptr, indices, data, (nr, nc))
        col0, bad = invert_col(col0, nr)
        col0[bad] = -1
    resolve = resolve_batched_sparse_free_rows if free_rows else resolve_batched_sparse
    col, _, ru, rv = resolve(
        torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
        torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
        torch.from_numpy(np.ascontiguousarray(data)).to(dev), (1, nr, nc), col0.to(dev),
        torch.zeros((1, nr), dtype=torch.float64, device=dev), v0.to(dev), with_cost=False, maximize=maximize)[:4]
    return single_result(col, tall, ru, rv)  # (the duals come back in the matrix's own signs)


# ---------------------------------------------------------------------------
# The k best assignments on the CSR (the lsap_murty_children_csr_
# and lsap_kbest_csr_ entries): kbest_batched on the densification, without the
# dense matrix.
# ---------------------------------------------------------------------------
def murty_children_batched_sparse(crow, col_indices, values, shape, col, v, p, forb, shapes=None,
                                  validate: bool = True, free_rows: bool = False):
    """murty_children_batched on sparse costs (the lsap_murty_children_csr_
    entries) -> (col int32 [B, NR, NR], cost float64 [B, NR], u [B, NR, NR],
    v [B, NR, NC], kept int32 [B, NR]): what murty_children_batched returns for
    the densification (densify) with the same shapes and the same node -- the
    same col and kept, the same bits in cost, u and v equal by value (a zero may
    carry the other sign) -- without building it.

    The batch, `shapes` and `validate` are solve_batched_sparse's, with NR <= NC
    <= SH_MAX_N; the node (col, v, p, forb) is murty_children_batched's: read as
    data and not modified.  A forced row whose column is not stored makes the
    child infeasible: col -1 and cost +inf, as for a child that does not
    exist.

    free_rows=True (the lsap_murty_children_fr_csr_ entries):
    what murty_children_batched(free_rows=True) returns for the densification;
    every child is the free-rows warm start of the padded M_t, whose virtual
    rows read no entry of the CSR."""
    crow, col_indices, values, shape, p_ = _sparse_batch(crow, col_indices, values, shape, shapes, validate,
                                                         limit=_lib.SH_MAX_N)
    B, NR, NC = shape
    W = forbidden_words(NC)
    if tuple(col.shape) != (B, NR) or tuple(v.shape) != (B, NC) or tuple(p.shape) != (B,) \
            or tuple(forb.shape) != (B, W):
        raise ValueError(f"expected col [{B}, {NR}], v [{B}, {NC}], p [{B}] and forb [{B}, {W}]")
    if v.dtype != torch.float64:
        raise TypeError(f"the duals of {values.dtype} costs are torch.float64")
    if forb.dtype != torch.int64:
        raise TypeError("forb holds its 64-bit words as torch.int64")
    for name, x in (("col", col), ("p", p)):
        if x.dtype not in _COL_DTYPES:
            raise TypeError(f"{name} must be an integer tensor, got {x.dtype}")
    dev = values.device
    if p_.empty:
        return (torch.full((B, NR, NR), -1, dtype=torch.int32, device=dev),
                torch.full((B, NR), float("inf"), dtype=torch.float64, device=dev),
                torch.zeros((B, NR, NR), dtype=torch.float64, device=dev),
                torch.zeros((B, NR, NC), dtype=torch.float64, device=dev),
                torch.zeros((B, NR), dtype=torch.int32, device=dev))
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p_, crow, col_indices, values, False)
    col0, v0, p0, f0 = narrow_col(col).contiguous(), v.contiguous(), narrow_col(p).contiguous(), forb.contiguous()
    ccol = torch.empty((B, NR, NR), dtype=torch.int32, device=dev)
    cost = torch.empty((B, NR), dtype=torch.float64, device=dev)
    cu = torch.empty((B, NR, NR), dtype=torch.float64, device=dev)
    cv = torch.empty((B, NR, NC), dtype=torch.float64, device=dev)
    kept = torch.empty((B, NR), dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(NR, NC, B))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nnz = values.numel()
    rc = getattr(L, ("lsap_murty_children_fr_csr_" if free_rows else "lsap_murty_children_csr_")
                 + DTYPE_SUFFIX[values.dtype])(
        _p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, NR, NC, B, _p(shape_dev), _p(col0),
        _p(v0), _p(p0), _p(f0), _p(ccol), _p(cost), _p(cu), _p(cv), _p(kept), _p(work), nbytes,
        _lib.SH_COMPAT_TIEBREAK, current_stream_handle(dev))
    _lib.check(rc, "lsap_murty_children_fr_csr" if free_rows else "lsap_murty_children_csr")
    return ccol, cost, cu, cv, kept


def kbest_batched_sparse(crow, col_indices=None, values=None, shape=None, k: int = 1, shapes=None,
                         maximize: bool = False, validate: bool = True, free_rows: bool = False):
    """kbest_batched on sparse costs, a missing entry being a forbidden pair
    (the lsap_kbest_csr_ entries) -> (cols int32 [B, k, NR], costs float64
    [B, k], count int32 [B]): cols, costs and count of kbest_batched on the
    densification (densify), the same integers and the same bits, in the same
    rank order, without building it.  Rank 0 is solve_batched_sparse's
    assignment.

    The batch, `shapes`, maximize and `validate` are solve_batched_sparse's (the
    triple with shape = (B, NR, NC), or one 2-D torch.sparse_csr tensor in place
    of crow), with 1 <= NR <= NC <= SH_MAX_N: ValueError for a tall batch, for a
    k that is no integer >= 1 and for a pool that does not fit.  One call
    launches 3 k kernels whatever the data, allocates its pool once and never
    synchronises.

    free_rows=True (the lsap_kbest_fr_csr_ entries): cols, costs
    and count of kbest_batched(free_rows=True) on the densification.  Every
    child is computed on the padded square problem; the ranks have the default
    mode's costs (equal bits wherever every sum is exact), and among
    assignments of equal cost the order and the choice may differ.  The same
    pool and the same 3 k launches.  When it pays (measured on the MI355X, 5 %
    density, k = 10, 1 and 64 instances): on wide instances a few
    rows short of square a child runs one search from 250 x 256 up (1.8 to 3.0
    for the root's children at 60 x 64) instead of 2 to 65, and a call
    takes 1.4x to 1.65x less time at 60 x 64, 2.5x to 2.6x less at 250 x 256
    and 4.9x to 5.8x less at 1018 x 1024; it stays 1.14x to 1.25x behind
    kbest_batched(free_rows=True) on a densification built beforehand.  Not
    measured with far fewer rows than columns, where the warm start's records
    say free rows loses."""
    crow, col_indices, values, shape, p = _sparse_batch(crow, col_indices, values, shape, shapes, validate,
                                                        limit=_lib.SH_MAX_N)
    if int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    k = int(k)
    B, NR, NC = shape
    dev = values.device
    if p.empty:
        return (torch.full((B, k, NR), -1, dtype=torch.int32, device=dev),
                torch.full((B, k), float("-inf") if maximize else float("inf"), dtype=torch.float64, device=dev),
                torch.zeros(B, dtype=torch.int32, device=dev))
    require_gpu()
    crow, col_indices, values, shape_dev = _sparse_operands(p, crow, col_indices, values, maximize)
    L = _lib.lib()
    nbytes = int(L.lsap_kbest_csr_work_bytes(NR, NC, B, k))
    if nbytes == 0:
        raise ValueError(f"k = {k} is too large for a [{B}, {NR}, {NC}] batch")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    cols = torch.empty((B, k, NR), dtype=torch.int32, device=dev)
    costs = torch.empty((B, k), dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    nnz = values.numel()
    rc = getattr(L, ("lsap_kbest_fr_csr_" if free_rows else "lsap_kbest_csr_") + DTYPE_SUFFIX[values.dtype])(
        _p(crow), _p(col_indices) if nnz else None, _p(values) if nnz else None, NR, NC, B, _p(shape_dev), k,
        _p(cols), _p(costs), _p(count), _p(work), nbytes, _lib.SH_COMPAT_TIEBREAK, current_stream_handle(dev))
    _lib.check(rc, "lsap_kbest_fr_csr" if free_rows else "lsap_kbest_csr")
    if maximize:
        costs = -costs
    return cols, costs, count


def kbest_assignments_sparse(A, k: int, maximize: bool = False, device: int | str = 0, free_rows: bool = False):
    """kbest_assignments for one sparse matrix whose missing entries are
    forbidden pairs -> (col_inds int64 [m, nr], costs float64 [m]), m <= k the
    number of assignments that exist, best first: those of kbest_assignments on
    densify(A).  A is linear_sum_assignment_sparse's, up to SH_MAX_N on the
    longer side; a tall matrix is solved as its transpose (csr_transpose) and
    col_inds has -1 for the rows left out.  A stored +inf (under maximize:
    -inf) is a missing entry; NaN and -inf (under maximize: +inf) raise
    ValueError.  free_rows is kbest_batched_sparse's."""
    indptr, indices, data, (nr, nc) = _csr_of(A)
    if int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    if nr == 0 or nc == 0:
        return np.zeros((0, nr), dtype=np.int64), np.zeros(0, dtype=np.float64)
    if max(nr, nc) > _lib.SH_MAX_N:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N}")
    if data.dtype not in (np.float64, np.float32):
        data = data.astype(np.float64)
    if np.isnan(data).any() or (data == (np.inf if maximize else -np.inf)).any():
        raise ValueError("matrix contains invalid numeric entries")
    NR = nr
    tall = nr > nc
    if tall:
        indptr, indices, data, (nr, nc) = csr_transpose(indptr, indices, data, (nr, nc))
    dev = device_of(device)
    if maximize:  # (negated here, so that the validation meets the forbidden value as +inf)
        data = -data
    cols, costs, count = kbest_batched_sparse(
        torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
        torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
        torch.from_numpy(np.ascontiguousarray(data)).to(dev), shape=(1, nr, nc), k=int(k), free_rows=free_rows)
    if maximize:
        costs = -costs
    if tall:
        cols = invert_tall(cols.view(int(k), nr), NR).view(1, int(k), NR)
    m = int(count[0])
    return cols[0, :m].cpu().numpy().astype(np.int64), costs[0, :m].cpu().numpy()


def maximum_bipartite_matching(A, device: int | str = 0):
    """scipy.sparse.csgraph.maximum_bipartite_matching(A, perm_type="column")
    on the GPU: an int64 numpy array [nr] with the column matched to each row, -1
    for a row without one.  Every stored entry is an edge, whatever its value,
    as in scipy.  A: the operands of linear_sum_assignment_sparse, up to
    SH_MAX_N_LARGE on the longer side; tall input is matched as its transpose
    and inverted.  The size of the matching is scipy's; which maximum matching
    it is, is not."""
    indptr, indices, _, (nr, nc) = _csr_of(A)
    if nr == 0 or nc == 0:
        return np.full(nr, -1, dtype=np.int64)
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    tall = nr > nc
    if tall:
        indptr, indices, _, (nr, nc) = csr_transpose(indptr, indices, np.zeros(indices.size), (nr, nc))
    dev = device_of(device)
    match, _, _ = maximum_matching_sparse(torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
                                          torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
                                          None, shape=(1, nr, nc))
    if tall:
        match = invert_tall(match, nc)
    return match[0].cpu().numpy().astype(np.int64)
