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
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .context import current_stream_handle, require_gpu
from .lsap import DTYPE_SUFFIX, _p, check_shapes, invert_tall, tall_result


def solve_bottleneck_batched(C: torch.Tensor, with_value: bool = True, flags: int = 0, shapes=None,
                             maximize: bool = False):
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
    does: ValueError for rank, size and shapes, TypeError for the dtype."""
    if C.dim() != 3:
        raise ValueError("expected [B, NR, NC]")
    B, NR, NC = C.shape
    if max(NR, NC) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(NR, NC) = {max(NR, NC)} > {_lib.SH_MAX_N_LARGE}")
    if C.dtype not in DTYPE_SUFFIX:
        raise TypeError(f"unsupported dtype {C.dtype}")
    shape_host = None
    if shapes is not None:
        if NR > NC:
            raise ValueError(f"a ragged batch must be padded wide, got [{NR}, {NC}]: "
                             "transpose the batch so that every instance has nr <= nc")
        shape_host = check_shapes(shapes, B, NR, NC)
    dev = C.device
    if B == 0 or NR == 0 or NC == 0:
        return (torch.full((B, NR), -1, dtype=torch.int32, device=dev),
                torch.zeros(B, dtype=C.dtype, device=dev) if with_value else None)
    require_gpu()
    shape_dev = torch.from_numpy(shape_host).to(dev) if shape_host is not None else None
    tall = NR > NC
    Cw = (C.transpose(1, 2) if tall else C).contiguous()
    _, nr, nc = Cw.shape
    col = torch.empty((B, nr), dtype=torch.int32, device=dev)
    value = torch.empty(B, dtype=C.dtype, device=dev) if with_value else None
    fl = flags | (_lib.SH_FLAG_MAXIMIZE if maximize else 0)
    rc = getattr(_lib.lib(), "lbap_solve_" + DTYPE_SUFFIX[C.dtype])(
        _p(Cw), nr, nc, B, _p(shape_dev), _p(col), _p(value), fl, current_stream_handle(dev))
    _lib.check(rc, "lbap_solve")
    return (invert_tall(col, NR) if tall else col), value


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


def linear_bottleneck_assignment(cost_matrix, maximize: bool = False, device: int | str = 0):
    """One matrix -> (row_ind, col_ind, value): the assignment of every row of
    the shorter side that minimises the largest chosen cost (maximises the
    smallest with maximize), row_ind and col_ind as
    scipy.optimize.linear_sum_assignment returns them (wide: arange(nr) and
    the columns; tall: the rows kept, sorted, with their columns), value a
    numpy scalar of the input's (widened) dtype equal to
    cost_matrix[row_ind, col_ind].max() (min with maximize).

    ValueError("matrix contains invalid numeric entries") on NaN,
    ValueError("cost matrix is infeasible") when no full matching of the
    shorter side avoids +inf (-inf with maximize)."""
    C = np.asarray(cost_matrix)
    if C.ndim != 2:
        raise ValueError("expected a matrix (2-D array), got a %r array" % (C.shape,))
    C = _widen(C)
    nr, nc = C.shape
    if nr == 0 or nc == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), C.dtype.type(0)
    if max(nr, nc) > _lib.SH_MAX_N_LARGE:
        raise ValueError(f"max(nr, nc) = {max(nr, nc)} > {_lib.SH_MAX_N_LARGE}")
    if np.issubdtype(C.dtype, np.floating) and np.isnan(C).any():
        raise ValueError("matrix contains invalid numeric entries")
    tall = nr > nc
    if tall:
        C = C.T
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    Ct = torch.from_numpy(np.ascontiguousarray(C)).to(dev)
    col, value = solve_bottleneck_batched(Ct.unsqueeze(0), maximize=maximize)
    col = col[0].cpu().numpy().astype(np.int64)
    if (col < 0).any():
        raise ValueError("cost matrix is infeasible")
    rows, cols = tall_result(col) if tall else (np.arange(col.size, dtype=np.int64), col)
    return rows, cols, value.cpu().numpy()[0]
