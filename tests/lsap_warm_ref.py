"""TEST INFRASTRUCTURE ONLY: the warm start of the batched LSAP solver on the
CPU, in numpy, for int64 and float64 matrices with nr <= nc.

`prologue(C, col0, v0)` is the definition of the start state,
implemented literally:

  1  v[j] = v0[j] inside the window (integers: -2^56 <= v0[j] <= 0; floats:
     finite and <= 0), else 0
  2  row4col: rows ascending, a row with 0 <= col0[i] < nc takes that column
     unless it is taken (the lowest row wins a duplicate)
  3  nr < nc: v = 0 on every column without a row
  4  u[i] = min_j (C[i, j] - v[j]), one subtraction per entry, min by value
  5  a pair (i, j) of step 2 is kept iff C[i, j] - v[j] == u[i]; otherwise it
     is dropped and, if nr < nc and v[j] < 0, the column enters the raise set
  6  while the set holds a column j: v[j] = 0, and every row with
     C[i, j] < u[i] takes u[i] = C[i, j] and loses its kept pair (i, j'), whose
     column enters the set if v[j'] < 0.  Each column is raised at most once.
  7  a float instance with u[i] = +inf in some row is infeasible (ValueError)

For nr == nc steps 3 and 6 are skipped.  The result of step 6 is a least fixed
point and does not depend on the order of the pops; `order` chooses between
two orders ("fifo", "lifo") so that a test can check that.

`replay_from(C, col4row, row4col, u, v)` is lsap_duals_ref.replay's loop started
from such a state: it skips every row that has a column.  Returns
(col4row, u, v, searches).  Zeros compare by value throughout, as on the GPU.
"""
from __future__ import annotations

import numpy as np

from lsap_duals_ref import _prepare, replay_state

V_MIN = -(1 << 56)


def sanitise(v0, dtype):
    v0 = np.asarray(v0)
    if np.issubdtype(dtype, np.integer):
        v0 = v0.astype(np.int64)
        return np.where((v0 >= V_MIN) & (v0 <= 0), v0, 0).astype(np.int64)
    v0 = v0.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v0) & (v0 <= 0), v0, 0.0).astype(np.float64)


def prologue(C, col0, v0, order="fifo"):
    """-> (col4row [nr], row4col [nc], u [nr], v [nc], kept)."""
    C, T, inf, nr, nc = _prepare(C)
    col0 = np.asarray(col0).astype(np.int64)
    assert col0.shape == (nr,) and np.asarray(v0).shape == (nc,)
    v = sanitise(v0, C.dtype)                                   # 1
    row4col = -np.ones(nc, dtype=np.int64)
    for i in range(nr):                                         # 2
        j = int(col0[i])
        if 0 <= j < nc and row4col[j] < 0:
            row4col[j] = i
    wide = nr < nc
    if wide:                                                    # 3
        v[row4col < 0] = 0
    with np.errstate(over="ignore", invalid="ignore"):
        red = C - v[None, :]                                    # 4
    u = red.min(axis=1)
    col4row = -np.ones(nr, dtype=np.int64)
    todo = []
    for j in range(nc):                                         # 5
        i = int(row4col[j])
        if i < 0:
            continue
        if red[i, j] == u[i]:
            col4row[i] = j
        else:
            row4col[j] = -1
            if wide and v[j] < 0:
                todo.append(j)
    if wide:                                                    # 6
        for _ in range(nc):  # (a column enters the set once: at most nc pops)
            if not todo:
                break
            j = todo.pop(0) if order == "fifo" else todo.pop()
            v[j] = 0
            for i in np.flatnonzero(C[:, j] < u):
                u[i] = C[i, j]
                jp = int(col4row[i])
                if jp >= 0:
                    col4row[i] = -1
                    row4col[jp] = -1
                    if v[jp] < 0:
                        todo.append(jp)
        assert not todo
    if not np.issubdtype(C.dtype, np.integer) and not (u < np.inf).all():   # 7
        raise ValueError("cost matrix is infeasible")
    return col4row, row4col, u, v, int((col4row >= 0).sum())


def replay_from(C, col4row, row4col, u, v):
    """lsap_duals_ref.replay's loop from a state; the state is not modified."""
    return replay_state(C, col4row, row4col, u, v)


def warm(C, col0, v0):
    """prologue + replay_from -> (col4row, u, v, kept, searches)."""
    c4r, r4c, u, v, kept = prologue(C, col0, v0)
    col, u, v, searches = replay_from(C, c4r, r4c, u, v)
    return col, u, v, kept, searches
