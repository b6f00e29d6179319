"""GPU linear bottleneck assignment (min-max matching), batched.

The sibling of lsap.py's min-sum solver: for each cost matrix, the assignment
of every row of the shorter side whose LARGEST chosen cost is as small as
possible; with maximize, the one whose smallest chosen cost is as large as
possible.  Same inputs and batching as solve_batched (square, wide, tall and
ragged batches, six dtypes, up to SH_MAX_N_LARGE = 4096 rows or columns),
through the lbap_solve_ entries of the C-ABI.

Costs are only compared, never added, so every dtype is solved exactly at its
own width and the value returned is an element of the input bit for bit.
Forbidden pairs are +inf and NaN of the floating-point dtypes (-inf and NaN
under maximize); integers have none.  Optima are far from unique: the solver
returns the one its search order defines, the same in every
kernel configuration, which tests/lbap_ref.py replays on the host.

An answer can be proved without that replay.  With witness=True the solver
also returns a Hall violator: rows R which the entries strictly below `value`
join to fewer than |R| columns, so that no assignment of every row stays below
`value`; check_bottleneck counts both on the device and flags == 0 proves an
instance optimal (flags == SH_LBCERT_NONE: infeasible), for every dtype and
the whole int64 range.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .context import current_stream_handle, require_gpu
from ._batch import (DTYPE_SUFFIX, _p, device_of, empty_result, invert_col, narrow_col, plan, single_empty,
                     single_result, tall_view, wide_view)


def solve_bottleneck_batched(C: torch.Tensor, with_value: bool = True, flags: int = 0, shapes=None,
                             maximize: bool = False, witness: bool = False):
    """C: device tensor [B, NR, NC] (int64 / int32 / float64 / float32 /
    float16 / bfloat16) -> (col int32 [B, NR], value [B] of C.dtype, or None
    without with_value).

    col[b, i] is the column of row i, -1 for a row without one: the NR - NC
    rows left out of a tall instance, every row of an infeasible instance
    (floating point only: no matching of the shorter side avoids +inf / NaN,
    or -inf / NaN under maximize) and the padded rows of a ragged one.
    value[b] is the bottleneck, max over the chosen entries (min under
    maximize), bit for bit an element of C; +inf (-inf under maximize) for an
    infeasible instance and 0 for an empty one.  -0.0 and +0.0 compare equal.

    `shapes` ([B, 2] integers, host or device) makes the batch ragged as in
    solve_batched: instance b is the top-left shapes[b] corner of its padded
    matrix, which must be wide; the padding is never read.  Tall batches
    (NR > NC) are solved as their transpose and inverted on the device.
    maximize reverses the order of the costs and never negates them.  There
    is no int64 range check and none is needed: the whole int64 range is
    solved exactly, INT64_MIN and INT64_MAX included.  Raises as solve_batched
    does: ValueError for rank, size and shapes, TypeError for the dtype.

    witness=True returns (col, value, wit) from the lbap_solve_wit_ entries,
    col and value the same bits.  wit (uint8) marks a Hall violator R with 1:
    the entries strictly below value[b] (above, under maximize) join the lines
    of R to fewer than |R| lines of the other side, which proves value[b]
    optimal; for an infeasible instance the same holds of the entries that are
    not forbidden.  wit is [B, min(NR, NC)] over the SHORTER side: rows of a
    wide batch, and, since a tall batch is solved as its transpose, [B, NC]
    over the columns of a tall one.  Padded rows and empty instances are 0."""
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE, shapes)
    dev = C.device
    if p.empty:
        empty = empty_result(p, with_value, False, C.dtype, dev)
        return empty + (torch.zeros((p.B, p.nr), dtype=torch.uint8, device=dev),) if witness else empty
    require_gpu()
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    Cw = (wide_view(C)[0] if p.tall else C).contiguous()
    col = torch.empty((p.B, p.nr), dtype=torch.int32, device=dev)
    value = torch.empty(p.B, dtype=C.dtype, device=dev) if with_value else None
    fl = flags | (_lib.SH_FLAG_MAXIMIZE if maximize else 0)
    if witness:
        wit = torch.empty((p.B, p.nr), dtype=torch.uint8, device=dev)
        rc = getattr(_lib.lib(), "lbap_solve_wit_" + DTYPE_SUFFIX[C.dtype])(
            _p(Cw), p.nr, p.nc, p.B, _p(shape_dev), _p(col), _p(value), _p(wit), fl, current_stream_handle(dev))
        _lib.check(rc, "lbap_solve_wit")
        return (tall_view(p, col)[0] if p.tall else col), value, wit
    rc = getattr(_lib.lib(), "lbap_solve_" + DTYPE_SUFFIX[C.dtype])(
        _p(Cw), p.nr, p.nc, p.B, _p(shape_dev), _p(col), _p(value), fl, current_stream_handle(dev))
    _lib.check(rc, "lbap_solve")
    return (tall_view(p, col)[0] if p.tall else col), value


def check_bottleneck(C: torch.Tensor, col: torch.Tensor, value: torch.Tensor, wit: torch.Tensor, shapes=None,
                     maximize: bool = False):
    """The certificate of a bottleneck solve, on the device (lbap_check_
    entries) -> (nR int32 [B], nN int32 [B], flags int32 [B]).

    C, col, value and wit as solve_bottleneck_batched(witness=True) takes and
    returns them: col [B, NR], value [B] of C.dtype, wit uint8 [B, min(NR, NC)].
    nR is the number of live lines marked in wit and nN the number of live lines
    of the other side that an entry strictly better than value[b] joins to one
    of them.  flags holds SH_LBCERT_* bits:
      COL      col is not an assignment of the live rows (integers: or is all -1)
      VALUE    value is not the largest chosen entry (smallest under maximize;
               -0.0 equals +0.0), or col is all -1 and value not the forbidden
               infinity
      WITNESS  not nN < nR: wit does not prove the value
      NONE     every live row has col == -1
    flags == 0 proves instance b optimal and flags == SH_LBCERT_NONE proves it
    infeasible, by comparisons alone: every dtype, int64 over its whole range.
    An empty instance gives 0 and (0, 0).  A tall batch is checked as its
    transpose, with col inverted on the device.  Raises as the solver does."""
    p = plan(C.shape, C.dtype, _lib.SH_MAX_N_LARGE, shapes)
    B, NR = p.B, p.NR
    if tuple(col.shape) != (B, NR) or tuple(value.shape) != (B,) or tuple(wit.shape) != (B, p.nr):
        raise ValueError(f"expected col [{B}, {NR}], value [{B}] and wit [{B}, {p.nr}]")
    if value.dtype != C.dtype or wit.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"value must be {C.dtype} and wit uint8 or bool")
    col = narrow_col(col)
    dev = C.device
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    if p.empty:
        return counts[:, 0], counts[:, 1], flags
    require_gpu()
    shape_dev = p.shapes_on(dev) if p.shapes is not None else None
    bad = None
    if p.tall:
        C, col, bad = wide_view(C)[0], *invert_col(col, p.NC)
    C, col, value = C.contiguous(), col.contiguous(), value.contiguous()
    wit = wit.to(torch.uint8).contiguous()
    rc = getattr(_lib.lib(), "lbap_check_" + DTYPE_SUFFIX[C.dtype])(
        _p(C), p.nr, p.nc, B, _p(shape_dev), _p(col), _p(value), _p(wit), _p(counts), _p(flags),
        _lib.SH_FLAG_MAXIMIZE if maximize else 0, current_stream_handle(dev))
    _lib.check(rc, "lbap_check")
    if bad is not None:  # a tall col that was no assignment before its inversion
        flags = flags | (bad.to(torch.int32) * _lib.SH_LBCERT_COL)
    return counts[:, 0], counts[:, 1], flags


def _widen(C: np.ndarray) -> np.ndarray:
    """The matrix in a dtype the solver takes: bool and unsigned integers widen
    to int64 (uint64 beyond int64: float64, as linear_sum_assignment does),
    other integers to int32 or int64, floats stay float16 / float32 / float64.
    Integers never pass through a float."""
    if C.dtype == np.bool_:
        return C.astype(np.int64)
    if np.issubdtype(C.dtype, np.unsignedinteger):
        if C.dtype == np.uint64 and C.size and int(C.max()) > np.iinfo(np.int64).max:
            return C.astype(np.float64)
        return C.astype(np.int64)
    if np.issubdtype(C.dtype, np.integer):
        return C if C.dtype in (np.int32, np.int64) else C.astype(np.int64)
    if C.dtype in (np.float16, np.float32, np.float64):
        return C
    if np.issubdtype(C.dtype, np.floating):
        return C.astype(np.float64)
    raise TypeError(f"unsupported dtype {C.dtype}")


def linear_bottleneck_assignment(cost_matrix, maximize: bool = False, device: int | str = 0,
                                 witness: bool = False):
    """One matrix -> (row_ind, col_ind, value): the assignment of every row of
    the shorter side that minimises the largest chosen cost (maximises the
    smallest with maximize), row_ind and col_ind as
    scipy.optimize.linear_sum_assignment returns them (wide: arange(nr) and
    the columns; tall: the rows kept, sorted, with their columns), value a
    numpy scalar of the input's (widened) dtype equal to
    cost_matrix[row_ind, col_ind].max() (min with maximize).

    witness=True returns (row_ind, col_ind, value, wit): wit a bool array over
    the shorter side (rows of a wide matrix, columns of a tall one) marking a
    Hall violator, the proof that no assignment beats value (see
    solve_bottleneck_batched and check_bottleneck).

    ValueError("matrix contains invalid numeric entries") on NaN,
    ValueError("cost matrix is infeasible") when no full matching of the
    shorter side avoids +inf (-inf with maximize)."""
    C = np.asarray(cost_matrix)
    if C.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %r array" % (C.shape,))
    C = _widen(C)
    nr, nc = C.shape
    if nr == 0 or nc == 0:
        return single_empty(nr, nc, False) + (C.dtype.type(0),) + ((np.zeros(0, dtype=bool),) if witness else ())
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    if np.issubdtype(C.dtype, np.floating) and np.isnan(C).any():
        raise ValueError("matrix contains invalid numeric entries")
    tall = nr > nc
    if tall:
        C = C.T
    Ct = torch.from_numpy(np.ascontiguousarray(C)).to(device_of(device))
    col, value, *wit = solve_bottleneck_batched(Ct.unsqueeze(0), maximize=maximize, witness=witness)
    res = single_result(col, tall)
    return res + (value.cpu().numpy()[0],) + ((wit[0][0].cpu().numpy().astype(bool),) if witness else ())
