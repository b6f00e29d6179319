"""TEST INFRASTRUCTURE ONLY: lsap_match_csr_ and lsap_check_hall_csr_ on the
host, written from the comment block above SH_HALL_MATCH in
include/santa_hip.h and from nothing else (no GPU, no library).

All three functions take ONE instance: the CSR rows of its padded NR x NC
matrix (indptr [NR + 1], indices, data or None) and shape = (nr_b, nc_b) of a
ragged member (None: the whole matrix).

  edges(...)      bool [NR, NC]: the stored entries of the live corner whose
                  value is not +inf (a NaN is an edge; no data: every stored one)
  match_ref(...)  (card, wit uint8 [NR]): the size of scipy's maximum matching
                  of the edges and the rows an alternating path reaches from an
                  unmatched live row; `order` permutes the rows scipy sees, so a
                  test can show that wit does not depend on the matching
  check_ref(...)  ((nM, nR, nN), flags) of a claimed (match, wit)
"""
import numpy as np

MATCH, WITNESS, DEFICIENT = 1, 2, 4


def shape_kind(NR, NC, shape):
    """(nr_b, nc_b, kind): kind "live", "empty" (nr_b == 0 inside the matrix) or "invalid"."""
    nr, nc = (NR, NC) if shape is None else (int(shape[0]), int(shape[1]))
    if 1 <= nr <= nc and nc <= NC and nr <= NR:
        return nr, nc, "live"
    return nr, nc, "empty" if nr == 0 and 0 <= nc <= NC else "invalid"


def edges(indptr, indices, data, NR, NC, shape=None):
    nr, nc, kind = shape_kind(NR, NC, shape)
    E = np.zeros((NR, NC), dtype=bool)
    if kind != "live":
        return E
    indptr = np.asarray(indptr, dtype=np.int64)
    e = np.arange(indptr[0], indptr[nr])                      # the stored entries of the live rows
    i = np.repeat(np.arange(nr), np.diff(indptr[:nr + 1]))
    j = np.asarray(indices, dtype=np.int64)[e]
    ok = (j >= 0) & (j < nc)
    if data is not None:
        ok &= ~(np.asarray(data)[e] == np.inf)
    E[i[ok], j[ok]] = True
    return E


def scipy_matching(E, order=None):
    """The column of each row (-1: none) of scipy's maximum matching of E, its
    rows presented in `order`."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    order = np.arange(E.shape[0]) if order is None else np.asarray(order)
    m = maximum_bipartite_matching(csr_matrix(E[order].astype(np.int8)), perm_type="column")
    out = np.full(E.shape[0], -1, dtype=np.int64)
    out[order] = m
    return out


def reachable_rows(E, match, nr):
    """uint8 [NR]: the live rows an alternating path (any edge from a row, the
    matched edge back from a column) reaches from an unmatched live row."""
    row_of = {int(c): i for i, c in enumerate(match[:nr]) if c >= 0}
    wit = np.zeros(E.shape[0], dtype=np.uint8)
    todo = [i for i in range(nr) if match[i] < 0]
    wit[todo] = 1
    seen = set()
    while todo:
        i = todo.pop()
        for j in np.flatnonzero(E[i]):
            if int(j) in seen:
                continue
            seen.add(int(j))
            k = row_of.get(int(j))   # (a free column here would mean the matching is not maximum)
            assert k is not None
            if not wit[k]:
                wit[k] = 1
                todo.append(k)
    return wit


def match_ref(indptr, indices, data, NR, NC, shape=None, order=None):
    nr, nc, kind = shape_kind(NR, NC, shape)
    if kind != "live":
        return 0, np.zeros(NR, dtype=np.uint8)
    E = edges(indptr, indices, data, NR, NC, shape)
    m = scipy_matching(E, order)
    return int((m >= 0).sum()), reachable_rows(E, m, nr)


def check_ref(indptr, indices, data, NR, NC, match, wit, shape=None):
    nr, nc, kind = shape_kind(NR, NC, shape)
    match = [int(c) for c in np.asarray(match)]
    if kind == "invalid":
        return (0, 0, 0), MATCH
    if kind == "empty":
        nr = 0
    E = edges(indptr, indices, data, NR, NC, shape)
    flags = 0
    if any(c != -1 for c in match[nr:]):
        flags |= MATCH                       # a padded row whose match is not -1
    live = match[:nr]
    nM = sum(c != -1 for c in live)
    ok = [c for c in live if c != -1 and 0 <= c < nc]
    if len(ok) != nM or len(set(ok)) != len(ok):
        flags |= MATCH                       # a value that is no column, or a column taken twice
    if any(0 <= c < nc and not E[i, c] for i, c in enumerate(live) if c != -1):
        flags |= MATCH                       # a pair that is no edge
    R = [i for i in range(nr) if np.asarray(wit)[i] != 0]
    nR = len(R)
    nN = int(E[R].any(axis=0).sum()) if R else 0
    if nR - nN != nr - nM:
        flags |= WITNESS
    if nM < nr:
        flags |= DEFICIENT
    return (nM, nR, nN), flags
