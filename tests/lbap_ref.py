"""Host references for the bottleneck assignment solver (no GPU, no library).

lbap_ref(C, maximize)        the normative loop of the lbap_solve_ entries
                             (include/santa_hip.h) in numpy,
                             vectorised over the columns: one search per row,
                             path length = largest cost on the path, the next
                             column the unvisited one with the least (path
                             length, taken, index).
threshold_value(C, maximize) the optimal bottleneck alone, by a method that
                             shares no code with the loop: the least distinct
                             cost t such that the graph of the entries <= t has
                             a matching of every row (scipy's Hopcroft-Karp).

Both compare costs by value (-0.0 == +0.0), take +inf and NaN of a float
matrix as forbidden, and reverse the order under maximize without negating an
integer: ~C for integers, -C for floats.  Matrices are nr x nc with nr <= nc.
"""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching


def _ordered(C, maximize):
    """(W, forbidden): W compares as the solver compares C (int64, or float64
    with the forbidden entries at +inf), and back(w) the element of C's dtype."""
    C = np.asarray(C)
    if np.issubdtype(C.dtype, np.integer):
        W = C.astype(np.int64)
        return (~W if maximize else W), np.zeros(C.shape, dtype=bool)
    W = C.astype(np.float64)
    if maximize:
        W = -W
    forb = np.isnan(W) | (W == np.inf)
    return np.where(forb, np.inf, W), forb


def _back(w, dtype, maximize):
    if np.issubdtype(dtype, np.integer):
        return dtype.type(~np.int64(w) if maximize else np.int64(w))
    return dtype.type(-w if maximize else w)


def _infeasible(nr, dtype, maximize):
    return np.full(nr, -1, dtype=np.int32), dtype.type(-np.inf if maximize else np.inf)


def lbap_ref(C, maximize=False):
    """-> (col int32 [nr], value (C.dtype scalar), max search steps, max hops)."""
    C = np.asarray(C)
    nr, nc = C.shape
    assert nr <= nc
    if nr == 0:
        return np.zeros(0, dtype=np.int32), C.dtype.type(0), 0, 0
    W, forb = _ordered(C, maximize)
    col4row = np.full(nr, -1, dtype=np.int64)
    row4col = np.full(nc, -1, dtype=np.int64)
    T = None
    max_steps = max_hops = 0
    idx = np.arange(nc)
    for cur in range(nr):
        spc = np.zeros(nc, dtype=W.dtype)
        reached = np.zeros(nc, dtype=bool)   # spc starts above every cost, the forbidden ones included
        spf = np.zeros(nc, dtype=bool)       # whether spc is a forbidden value
        path = np.full(nc, -1, dtype=np.int64)
        unvis = np.ones(nc, dtype=bool)
        i, mv, mvf, steps, sink = cur, None, False, 0, -1
        while True:
            steps += 1
            r = W[i] if mv is None else np.maximum(W[i], mv)
            rf = forb[i] | mvf
            # strict <, a forbidden value above every cost and equal to itself
            less = ~reached | (~rf & spf) | (~rf & ~spf & (r < spc))
            upd = unvis & less
            spc[upd], spf[upd], path[upd], reached[upd] = r[upd], rf[upd], i, True
            if not unvis.any():
                return _infeasible(nr, C.dtype, maximize) + (max_steps, max_hops)
            cand = unvis & ~spf
            if not cand.any():
                return _infeasible(nr, C.dtype, maximize) + (max_steps, max_hops)
            m = spc[cand].min()
            cand &= spc == m
            free = cand & (row4col < 0)
            j = int(idx[free][0]) if free.any() else int(idx[cand][0])
            mv, mvf = spc[j], False
            unvis[j] = False
            if row4col[j] < 0:
                sink = j
                break
            i = int(row4col[j])
        T = mv if T is None else max(T, mv)
        max_steps = max(max_steps, steps)
        hops, j = 0, sink
        while True:
            hops += 1
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
        max_hops = max(max_hops, hops)
    return col4row.astype(np.int32), _back(T, C.dtype, maximize), max_steps, max_hops


def threshold_value(C, maximize=False):
    """The optimal bottleneck of C as a C.dtype scalar (+inf, or -inf under
    maximize, when no matching of every row avoids the forbidden entries)."""
    C = np.asarray(C)
    nr, nc = C.shape
    assert 1 <= nr <= nc
    W, forb = _ordered(C, maximize)
    ok = ~forb

    def edges(mask):
        ii, jj = np.nonzero(mask)
        return ii, jj, W[ii, jj]

    def feasible(t):
        m = ww <= t
        g = csr_matrix((np.ones(int(m.sum()), dtype=np.int8), (ii[m], jj[m])), shape=(nr, nc))
        return int((maximum_bipartite_matching(g, perm_type="column") >= 0).sum()) == nr

    # A large matrix: if its 64 nc least entries already hold a matching of
    # every row, no larger cost can be the answer and the search runs on those.
    k = 64 * nc
    ii = None
    if W.size > 4 * k:
        cut = np.partition(W.ravel(), k)[k]
        ii, jj, ww = edges(ok & (W <= cut))
        if not (ww.size and feasible(cut)):
            ii = None
    if ii is None:
        ii, jj, ww = edges(ok)
    vals = np.unique(ww)
    if vals.size == 0 or not feasible(vals[-1]):
        return C.dtype.type(-np.inf if maximize else np.inf)
    # every row needs its own least entry: start there and gallop upwards, so
    # that the graphs tried stay about as sparse as the answer's
    # (W is float64 wherever something is forbidden: integers never meet the inf)
    lo = int(np.searchsorted(vals, (np.where(ok, W, np.inf) if forb.any() else W).min(axis=1).max()))
    lo = min(lo, vals.size - 1)
    step, hi = 1, lo
    while not feasible(vals[hi]):
        lo = hi + 1
        hi = min(hi + step, vals.size - 1)
        step *= 2
    while lo < hi:  # the least feasible index in [lo, hi]
        mid = (lo + hi) // 2
        if feasible(vals[mid]):
            hi = mid
        else:
            lo = mid + 1
    return _back(vals[lo], C.dtype, maximize)
