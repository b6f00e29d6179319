"""The host side that the batched assignment front ends share (lsap.py, lbap.py).

`plan` makes the argument checks of a padded [B, NR, NC] batch and returns the
immutable `Batch` record that everything else here reads; `single_result` is
the tail of the single-matrix front ends.  Nothing in this module asks for the
GPU or calls the library.  Every entry takes one order: argument checks, the
empty-batch answer, require_gpu(), the work.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

# every cost dtype -> the suffix of its C-ABI entries
DTYPE_SUFFIX = {torch.int64: "i64", torch.int32: "i32", torch.float64: "f64", torch.float32: "f32",
                torch.float16: "f16", torch.bfloat16: "bf16"}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def device_of(device: int | str) -> torch.device:
    return torch.device("cuda", device) if isinstance(device, int) else torch.device(device)


# ---------------------------------------------------------------------------
# Pure helpers on shapes and assignments.
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
_COL_DTYPES = (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8)


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
    if col.dtype in _COL_DTYPES:
        return col.to(torch.int32)
    raise TypeError(f"col must be an integer tensor, got {col.dtype}")


def tall_result(col_t):
    """scipy's (row_ind, col_ind) of a tall matrix from the solution col_t of
    its transpose: rows sorted ascending, each with its column."""
    col_t = np.asarray(col_t, dtype=np.int64)
    order = np.argsort(col_t)
    return col_t[order], order.astype(np.int64)


# ---------------------------------------------------------------------------
# One batched call.
# ---------------------------------------------------------------------------
class Batch(NamedTuple):
    """What the argument checks of a batched call establish (plan)."""
    B: int
    NR: int
    NC: int
    tall: bool                    # NR > NC: solved or checked as the transpose
    shapes: Optional[np.ndarray]  # check_shapes' int32 [B, 2] on the host; None: not ragged
    ddt: torch.dtype              # the duals' dtype: int64 for integer costs, float64 otherwise
    empty: bool                   # no instance or no entry: answered without the GPU
    nr: int                       # rows and
    nc: int                       # columns of the wide problem: min and max of (NR, NC)

    def shapes_on(self, dev):
        """The shapes (the batch is ragged) as the C entries read them, on dev."""
        return torch.from_numpy(self.shapes).to(dev)


_DUALS_DTYPE = {dt: torch.float64 if dt.is_floating_point else torch.int64 for dt in DTYPE_SUFFIX}


def plan(shape, dtype: torch.dtype, limit: int, shapes=None) -> Batch:
    """The argument checks of a padded batch of `shape` and cost `dtype`, at
    most `limit` rows or columns, ragged by `shapes` (or None) -> its Batch.
    ValueError for rank, size and shapes, TypeError for the dtype."""
    if len(shape) != 3:
        raise ValueError("expected [B, NR, NC]")
    B, NR, NC = shape
    tall = NR > NC
    nr, nc = (NC, NR) if tall else (NR, NC)
    if nc > limit:
        raise ValueError(f"max(NR, NC) = {nc} > {limit}")
    ddt = _DUALS_DTYPE.get(dtype)
    if ddt is None:
        raise TypeError(f"unsupported dtype {dtype}")
    if shapes is not None:
        if tall:
            raise ValueError(f"a ragged batch must be padded wide, got [{NR}, {NC}]: "
                             "transpose the batch so that every instance has nr <= nc")
        shapes = check_shapes(shapes, B, NR, NC)
    return Batch(B, NR, NC, tall, shapes, ddt, B == 0 or nr == 0, nr, nc)


def check_solution(p: Batch, cost_dtype, col, u, v) -> None:
    """A previous or claimed solution (col, u, v) of the batch: ValueError
    unless col and u are [B, NR] and v [B, NC], TypeError unless the duals have
    the batch's dual dtype and col an integer one.  No device work: the caller
    narrows col (narrow_col) after the empty-batch answer."""
    B, NR, NC = p.B, p.NR, p.NC
    if tuple(col.shape) != (B, NR) or tuple(u.shape) != (B, NR) or tuple(v.shape) != (B, NC):
        raise ValueError(f"expected col and u of shape [{B}, {NR}] and v of shape [{B}, {NC}]")
    if u.dtype != p.ddt or v.dtype != p.ddt:
        raise TypeError(f"the duals of {cost_dtype} costs are {p.ddt}")
    if col.dtype not in _COL_DTYPES:
        narrow_col(col)  # (raises its TypeError)


def empty_result(p: Batch, with_cost: bool, duals: bool, cost_dtype, dev):
    """The answer to an empty batch: (col, cost or None), with duals (col, cost,
    u, v); every row without a column, cost and duals 0."""
    out = (torch.full((p.B, p.NR), -1, dtype=torch.int32, device=dev),
           torch.zeros(p.B, dtype=cost_dtype, device=dev) if with_cost else None)
    if duals:
        out += (torch.zeros((p.B, p.NR), dtype=p.ddt, device=dev), torch.zeros((p.B, p.NC), dtype=p.ddt, device=dev))
    return out


def minimised(C, *duals):
    """(C, *duals) of the problem to minimise under maximize: each negated.  (This
    and the next two are called under `if maximize:` / `if p.tall:` only.)"""
    # (int32: -INT32_MIN wraps, so widen; the int64 bound covers int64)
    return (-(C.to(torch.int64) if C.dtype == torch.int32 else C), *(-d for d in duals))


def wide_view(C, u=None, v=None):
    """(C, u, v) of a tall batch as the wide problem it is solved or checked as:
    the transpose (a view), where the rows' duals belong to the columns.  (A col
    that comes in: invert_col, whose `bad` mask is the caller's to use.)"""
    return C.transpose(1, 2), v, u


def tall_view(p: Batch, col, u=None, v=None):
    """(col, u, v) of a tall batch from the results of its wide problem."""
    return invert_tall(col, p.NR), v, u


def alloc_outputs(p: Batch, with_cost: bool, duals: bool, cost_dtype, dev):
    """Unwritten (col, cost, u, v) of the wide problem; cost, u and v None
    where they are not asked for."""
    return (torch.empty((p.B, p.nr), dtype=torch.int32, device=dev),
            torch.empty(p.B, dtype=cost_dtype, device=dev) if with_cost else None,
            torch.empty((p.B, p.nr), dtype=p.ddt, device=dev) if duals else None,
            torch.empty((p.B, p.nc), dtype=p.ddt, device=dev) if duals else None)


def single_empty(nr: int, nc: int, duals: bool, dtype=np.int64):
    """A single-matrix front end's answer to an empty matrix (duals: zeros [nr] and [nc])."""
    z = np.zeros(0, dtype=np.int64)
    return (z, z.copy(), np.zeros(nr, dtype=dtype), np.zeros(nc, dtype=dtype)) if duals else (z, z.copy())


def single_result(col, tall: bool, u=None, v=None, negate: bool = False):
    """The tail of a single-matrix front end, from the batch of one that was
    solved wide: scipy's (row_ind, col_ind), with u also the duals in the
    matrix's own roles (negated back for a problem that went down negated).
    ValueError for an infeasible matrix."""
    col = col[0].cpu().numpy().astype(np.int64)
    if (col < 0).any():
        raise ValueError("cost matrix is infeasible")
    res = tall_result(col) if tall else (np.arange(col.size, dtype=np.int64), col)
    if u is None:
        return res
    u, v = u[0].cpu().numpy(), v[0].cpu().numpy()
    if negate:
        u, v = -u, -v
    return res + ((v, u) if tall else (u, v))
