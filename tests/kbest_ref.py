"""TEST INFRASTRUCTURE ONLY: the k best assignments of one float matrix
(nr <= nc) on the CPU, in numpy: Murty's partition in fixed row order, written
as its definition over lsap_duals_ref.replay (the root) and
lsap_warm_ref.warm (every child).

A node is (col [nr], v [nc], p, F bool [nc], cost).  Child t of a node,
p <= t < nr, is warm(masked(C, col, t, F_t), col, v) with
F_t = (F if t == p else {}) + {col[t]}; a child whose matrix is infeasible
does not exist.  Rank r is the node of least cost by value among those not yet
emitted, the one created first on a tie (the root, then by round, then by t).

`tail_sum` adds the chosen costs in the order of the GPU kernels' cost tail
(lane l adds its rows l, l + 64, ... in turn, then a butterfly over the 64
lanes), so that costs can be compared as bits for any input.
"""
from __future__ import annotations

import numpy as np

from lsap_duals_ref import replay
from lsap_warm_ref import warm


def tail_sum(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros(64, dtype=np.float64)
    for i in range(x.size):
        acc[i % 64] = acc[i % 64] + x[i]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return float(acc[0])


def forbidden_t(col, p, F, t):
    """F_t as a bool [nc]: F if t == p, and col[t] where that is a column."""
    nc = F.size
    Ft = F.copy() if t == p else np.zeros(nc, dtype=bool)
    if 0 <= col[t] < nc:
        Ft[col[t]] = True
    return Ft


def masked(C, col, t, Ft):
    """M_t of a node with assignment col, as a float64 matrix."""
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    M = C.copy()
    for i in range(t):
        M[i, :] = np.inf
        if 0 <= col[i] < nc:
            M[i, col[i]] = C[i, col[i]]
            M[t:, col[i]] = np.inf
    M[t, Ft] = np.inf
    return M


def child(C, col, v, p, F, t):
    """Child t of the node (col, v, p, F) -> (col, u, v, kept, searches, F_t),
    or None where it does not exist."""
    nr = len(col)
    if p < 0 or t < p or t >= nr:
        return None
    Ft = forbidden_t(col, p, F, t)
    try:
        c, u, v2, kept, searches = warm(masked(C, col, t, Ft), col, v)
    except ValueError:
        return None
    return c, u, v2, kept, searches, Ft


def kbest(C, k):
    """-> (cols int64 [k, nr], costs float64 [k], count, searches, trace): the
    ranks beyond count hold -1 and +inf; searches lists the Dijkstras of every
    child that exists, in creation order; trace[r] says where rank r came from:
    None for the root, else (col, v, p, F, t) -- child t of that node."""
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    cols = -np.ones((k, nr), dtype=np.int64)
    costs = np.full(k, np.inf)
    searches = []
    trace = []
    nodes = []  # [cost, col, v, p, F, origin], None once emitted; creation order
    try:
        col, _, v = replay(C)
        nodes.append([tail_sum(C[np.arange(nr), col]), col, v, 0, np.zeros(nc, dtype=bool), None])
    except ValueError:
        pass
    for r in range(k):
        live = [x for x in nodes if x is not None]
        if not live:
            return cols, costs, r, searches, trace
        best = min(x[0] for x in live)
        at = next(i for i, x in enumerate(nodes) if x is not None and x[0] == best)
        cost, col, v, p, F, origin = nodes[at]
        trace.append(origin)
        nodes[at] = None
        cols[r], costs[r] = col, cost
        if r == k - 1:
            break
        for t in range(p, nr):
            ch = child(C, col, v, p, F, t)
            if ch is not None:
                c, _, v2, _, s, Ft = ch
                searches.append(s)
                nodes.append([tail_sum(C[np.arange(nr), c]), c, v2, t, Ft, (col, v, p, F, t)])
    return cols, costs, k, searches, trace
