"""Host references for the bottleneck solver's Hall-violator witness and its
certificate (no GPU, no library).

lbap_witness_ref(C, maximize)   the loop of lbap_ref with the normative witness
                                rule -> (col, value, wit uint8 [nr]).  Search 0
                                counts as a rise, a later search only when its
                                final path length is STRICTLY above every
                                earlier one's.  At a rise R = {cur} and the rows
                                (of the matching before the augmentation) of the
                                visited columns whose path length is below the
                                final one; at a failed search R = {cur} and the
                                rows of every visited column.
lbap_check_ref(C, col, value, wit, maximize, shape=None)
                                the certificate of lbap_check_ in vectorised
                                numpy on unsigned keys -> (nR, nN, flags).  It
                                shares no code with the loop: keys are built
                                from the bits here, the loop compares values.

`rise` lets a test swap the rule (tie_no_rewrite pins that `>=` differs).
"""
import numpy as np

from lbap_ref import _back, _infeasible, _ordered

SH_LBCERT_COL = 1
SH_LBCERT_VALUE = 2
SH_LBCERT_WITNESS = 4
SH_LBCERT_NONE = 8

_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_SIGN = np.uint64(1 << 63)


def lbap_witness_ref(C, maximize=False, rise=lambda mv, top: mv > top):
    """-> (col int32 [nr], value (C.dtype scalar), wit uint8 [nr])."""
    C = np.asarray(C)
    nr, nc = C.shape
    assert nr <= nc
    wit = np.zeros(nr, dtype=np.uint8)
    if nr == 0:
        return np.zeros(0, dtype=np.int32), C.dtype.type(0), wit
    W, forb = _ordered(C, maximize)
    col4row = np.full(nr, -1, dtype=np.int64)
    row4col = np.full(nc, -1, dtype=np.int64)
    T = None
    idx = np.arange(nc)

    def mark(cur, cols):
        wit[:] = 0
        wit[cur] = 1
        wit[row4col[cols]] = 1

    for cur in range(nr):
        spc = np.zeros(nc, dtype=W.dtype)
        reached = np.zeros(nc, dtype=bool)
        spf = np.zeros(nc, dtype=bool)
        path = np.full(nc, -1, dtype=np.int64)
        unvis = np.ones(nc, dtype=bool)
        i, mv, mvf, sink = cur, None, False, -1
        while True:
            r = W[i] if mv is None else np.maximum(W[i], mv)
            rf = forb[i] | mvf
            less = ~reached | (~rf & spf) | (~rf & ~spf & (r < spc))
            upd = unvis & less
            spc[upd], spf[upd], path[upd], reached[upd] = r[upd], rf[upd], i, True
            cand = unvis & ~spf
            if not cand.any():  # no column left, or only forbidden entries lead on
                mark(cur, ~unvis)
                return _infeasible(nr, C.dtype, maximize) + (wit,)
            m = spc[cand].min()
            cand &= spc == m
            free = cand & (row4col < 0)
            j = int(idx[free][0]) if free.any() else int(idx[cand][0])
            mv = spc[j]
            unvis[j] = False
            if row4col[j] < 0:
                sink = j
                break
            i = int(row4col[j])
        if T is None or rise(mv, T):
            mark(cur, ~unvis & (spc < mv))  # (the visited columns are never at a forbidden length)
        T = mv if T is None else max(T, mv)
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row.astype(np.int32), _back(T, C.dtype, maximize), wit


def _keys(X, maximize):
    """lbap_key of every element as uint64 (the narrower dtypes keep their
    order when widened): integers bits ^ sign; floats -0.0 as +0.0, the
    sign-magnitude flip, NaN and the forbidden infinity all ones; maximize
    one more XOR with all ones."""
    X = np.asarray(X)
    if np.issubdtype(X.dtype, np.integer):
        k = X.astype(np.int64).view(np.uint64) ^ _SIGN
        return ~k if maximize else k
    F = np.array(X, dtype=np.float64)  # (a copy: float16 and float32 widen exactly)
    F[F == 0] = 0.0
    bits = F.view(np.uint64)
    k = np.where(bits & _SIGN != 0, ~bits, bits | _SIGN)
    if maximize:
        k = ~k
    return np.where(np.isnan(F) | (F == (-np.inf if maximize else np.inf)), _ONES, k)


def _is_forbidden_infinity(value, maximize):
    v = np.asarray(value)
    return bool(np.issubdtype(v.dtype, np.floating) and v == (-np.inf if maximize else np.inf))


def lbap_check_ref(C, col, value, wit, maximize=False, shape=None):
    """C [NR, NC] (padded when `shape` = (nr, nc) is given), col [NR] integers,
    value a scalar of C's dtype, wit [NR] bytes -> (nR, nN, flags)."""
    C = np.asarray(C)
    NR, NC = C.shape
    col = np.asarray(col).astype(np.int64)
    wit = np.asarray(wit)
    nr, nc = (NR, NC) if shape is None else (int(shape[0]), int(shape[1]))
    if not (1 <= nr <= nc <= NC and nr <= NR):
        if not (nr == 0 and 0 <= nc <= NC):
            return 0, 0, SH_LBCERT_COL  # not a shape of this matrix
        return 0, 0, (SH_LBCERT_COL if (col != -1).any() else 0)  # an empty instance
    flags = 0
    if (col[nr:] != -1).any():
        flags |= SH_LBCERT_COL
    live = col[:nr]
    none = live == -1
    valid = (live >= 0) & (live < nc)
    if (~none & ~valid).any() or np.unique(live[valid]).size != int(valid.sum()):
        flags |= SH_LBCERT_COL
    if none.all():
        flags |= SH_LBCERT_NONE
        if np.issubdtype(C.dtype, np.integer):
            flags |= SH_LBCERT_COL  # integers have no infeasible instance
    elif none.any():
        flags |= SH_LBCERT_COL
    K = _keys(C[:nr, :nc], maximize)
    vk = _keys(np.asarray(value, dtype=C.dtype).reshape(1), maximize)[0]
    if valid.any():
        if K[np.nonzero(valid)[0], live[valid]].max() != vk:
            flags |= SH_LBCERT_VALUE
    elif not _is_forbidden_infinity(np.asarray(value, dtype=C.dtype), maximize):
        flags |= SH_LBCERT_VALUE
    R = wit[:nr] != 0
    nR = int(R.sum())
    nN = int((K[R] < vk).any(axis=0).sum()) if nR else 0
    if not nN < nR:
        flags |= SH_LBCERT_WITNESS
    return nR, nN, flags
