"""TEST INFRASTRUCTURE ONLY: lsap_check_duals_csr_ on the host: the dense
certificate's reference (lsap_cert_ref.cert_ref) on the densification of ONE
instance, plus the rule the header adds for duals that are not finite.

csr_cert_ref(indptr, indices, data, NR, NC, col, u, v, shape=None) ->
(slack [3] float64, flags): indptr [NR + 1], indices, data are the instance's
own CSR rows; a missing entry is +inf, stored values are widened to float64.
"""
import numpy as np

from lsap_cert_ref import NONE, SLACK, cert_ref


def densify_one(indptr, indices, data, NR, NC):
    D = np.full((NR, NC), np.inf)
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(NR), np.diff(indptr))
    idx = np.asarray(indices, dtype=np.int64)[indptr[0]:indptr[NR]]
    val = np.asarray(data)[indptr[0]:indptr[NR]].astype(np.float64)
    ok = (idx >= 0) & (idx < NC)   # (an index outside the matrix is no entry)
    D[rows[ok], idx[ok]] = val[ok]
    return D


def csr_cert_ref(indptr, indices, data, NR, NC, col, u, v, shape=None):
    D = densify_one(indptr, indices, data, NR, NC)
    smin, tmax, gap, flags = cert_ref(D, col, u, v, shape)
    nr, nc = (NR, NC) if shape is None else (int(shape[0]), int(shape[1]))
    invalid = not (1 <= nr <= nc <= NC and nr <= NR) and not (nr == 0 and 0 <= nc <= NC)
    if not invalid and not flags & NONE:
        live = np.concatenate([np.asarray(u, dtype=np.float64)[:nr], np.asarray(v, dtype=np.float64)[:nc]])
        if not np.isfinite(live).all():
            smin, flags = np.float64(np.nan), flags | SLACK
    return np.array([smin, tmax, gap], dtype=np.float64), int(flags)
