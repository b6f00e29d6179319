"""TEST INFRASTRUCTURE ONLY: the free-rows warm start on the
CPU, in numpy, for int64 and float64 matrices with nr <= nc.

A wide instance is solved as the PADDED problem, vstack(C, zeros((nc - nr,
nc))): a square instance with nc - nr virtual rows of cost 0.  The mode is
defined by the existing definitions (lsap_warm_ref.prologue, replay_from)
applied to that written-out matrix:

  a  steps 1, 2, 4, 5 and 7 of lsap_warm_ref.prologue on the real rows -- the
     square path's steps, whatever nr: no column dual is raised
  b  m = min_j (0 - v[j]) (step 4 on a row of zeros; theta = 0 - m = max_j v[j]);
     the columns that are free after step 5 and have 0 - v[j] == m (step 5's
     test of a virtual pair, by value) go, ascending, to the virtual rows nr,
     nr + 1, ... while both last; every virtual row gets u = m
  c  replay_from on that state: one search for each row without a column, real
     rows first, then virtual rows, ascending

`start_state` builds (a, b) and asserts that it is exactly what
lsap_warm_ref.prologue returns for the padded matrix when col0 is the kept real
pairs extended by the columns of b.  `resolve` is the whole mode; `child` and
`kbest` are kbest_ref's with every child computed this way.

Integer costs with nr < nc return the normalised duals u + theta, v - theta
(exact; v <= 0 and v == 0 on every free column: lsap_duals_ref.invariants on
the unpadded matrix).  Float costs return the padded problem's duals as they
are.  A square instance is lsap_warm_ref.warm, duals and all.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import lsap_warm_ref as W
from lsap_duals_ref import _prepare


class FreeRows(NamedTuple):
    col: np.ndarray     # [nr] the real rows' columns
    u: np.ndarray       # [nr]
    v: np.ndarray       # [nc]
    cost: object        # summed over the real rows
    kept: int           # real pairs of col0 that were kept
    kept_free: int      # virtual pairs of the start state
    theta: object       # max_j v[j] of the padded problem's final state
    searches: int       # (nr - kept) + (nc - nr - kept_free)


def padded(C):
    C, _, _, nr, nc = _prepare(C)
    return np.vstack([C, np.zeros((nc - nr, nc), dtype=C.dtype)])


def neg_theta(v):
    """m = min_j (0 - v[j]), in v's dtype (+0.0 for a float zero of either sign)."""
    v = np.asarray(v)
    return (v.dtype.type(0) - v).min()


def start_state(C, col0, v0, virtual=None):
    """-> (P, col4row [nc], row4col [nc], u [nc], v [nc], kept, kept_free): the
    padded matrix and its start state.  virtual: the one row every virtual row
    is (zeros; a Murty child closes the forced columns with +inf)."""
    C, T, _, nr, nc = _prepare(C)
    P = padded(C)
    if virtual is not None:
        P[nr:] = virtual
    none = -np.ones(nc - nr, dtype=np.int64)
    # a: the padded matrix is square, so prologue skips steps 3 and 6; virtual rows that name no column change nothing
    # for the real ones
    c4r, r4c, u, v, kept = W.prologue(P, np.concatenate([np.asarray(col0).astype(np.int64), none]), v0)
    assert (c4r[nr:] < 0).all() and kept == int((c4r[:nr] >= 0).sum())
    kept_free = 0
    if nr < nc:
        with np.errstate(invalid="ignore"):
            d = P[nr] - v                                              # b (0 - v[j]; +inf on a closed column)
        m = d.min()
        assert (u[nr:] == m).all() and (virtual is not None or m == neg_theta(v))
        at_theta = np.flatnonzero((r4c < 0) & (d == m))[:nc - nr]
        kept_free = at_theta.size
        c4r[nr:nr + kept_free] = at_theta
        r4c[at_theta] = nr + np.arange(kept_free)
    # ... which is the prologue of the padded matrix from the kept pairs extended by those columns
    c4r2, r4c2, u2, v2, kept2 = W.prologue(P, c4r.copy(), v0)
    assert np.array_equal(c4r2, c4r) and np.array_equal(r4c2, r4c) and kept2 == kept + kept_free
    assert u2.tobytes() == u.tobytes() and v2.tobytes() == v.tobytes()
    return P, c4r, r4c, u, v, kept, kept_free


def resolve(C, col0, v0) -> FreeRows:
    C, T, _, nr, nc = _prepare(C)
    P, c4r, r4c, u, v, kept, kept_free = start_state(C, col0, v0)
    col, u, v, searches = W.replay_from(P, c4r, r4c, u, v)             # c
    assert searches == (nr - kept) + (nc - nr - kept_free)
    theta = T(0) - neg_theta(v)
    cost = C[np.arange(nr), col[:nr]].sum()
    u = u[:nr]
    if np.issubdtype(C.dtype, np.integer) and nr < nc:
        u, v = u + theta, v - theta
    return FreeRows(col[:nr], u, v, cost, kept, kept_free, theta, searches)


# --------------------------------------------------------------------------- Murty's partition with free rows
def child(C, col, v, p, F, t):
    """kbest_ref.child with free rows: child t of the node (col, v, p, F) is
    the free-rows warm start of M_t, whose virtual rows are rows > t: 0, and
    +inf on the columns the rows < t force -> (col [nr], u [nr], v [nc], kept,
    searches, F_t), or None where it does not exist."""
    import kbest_ref as K
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    if p < 0 or t < p or t >= nr:
        return None
    Ft = K.forbidden_t(col, p, F, t)
    virtual = np.zeros(nc)
    virtual[[int(c) for c in col[:t] if 0 <= c < nc]] = np.inf
    try:
        P, c4r, r4c, u, v2, kept, kept_free = start_state(K.masked(C, col, t, Ft), col, v, virtual)
        c, u, v2, searches = W.replay_from(P, c4r, r4c, u, v2)
    except ValueError:
        return None
    assert searches == (nr - kept) + (nc - nr - kept_free)
    return c[:nr], u[:nr], v2, kept, searches, Ft


def kbest(C, k):
    """kbest_ref.kbest with the children above (its loop, its ranks, its tie
    rule) -> (cols, costs, count, searches, trace)."""
    import kbest_ref as K
    C = np.asarray(C, dtype=np.float64)
    nr, nc = C.shape
    cols = -np.ones((k, nr), dtype=np.int64)
    costs = np.full(k, np.inf)
    searches, trace, nodes = [], [], []
    try:
        col, _, v = K.replay(C)
        nodes.append([K.tail_sum(C[np.arange(nr), col]), col, v, 0, np.zeros(nc, dtype=bool), None])
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
                nodes.append([K.tail_sum(C[np.arange(nr), c]), c, v2, t, Ft, (col, v, p, F, t)])
    return cols, costs, k, searches, trace
