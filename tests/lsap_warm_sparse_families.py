"""TEST INFRASTRUCTURE ONLY: warm-start cases of the sparse (CSR) batched LSAP
solver, in pure numpy.

The source batches are lsap_sparse_families' own: the same instances at the
same SHAPES (`cases()` is its case list), so every seam of the launch table is
crossed.  The previous state of an instance is the cold solution (col, v) of
the UNPERTURBED instance (lsap_sparse_families.expected: NaN duals and -1 for
an infeasible one, which a warm start reads as data like anything else).

`perturbed(family, nr, nc)` changes up to four distinct live rows of every
feasible instance with at least four live rows, inside its corner only:

  (a)  a chosen entry is made dearer (+ 37)
  (b)  a stored unchosen entry is made the row's cheapest (its least stored
       value less one)
  (c)  a chosen entry is REMOVED from the pattern (a Murty child)
  (d)  a MISSING entry is added with value 0

(a) and (c) take the first two rows of a seeded permutation of the live rows,
(b) and (d) the next rows that have a stored unchosen, respectively a missing,
entry in the corner (a row of `full` has no missing entry: (d) is then left
out).  Instances that are infeasible, or have fewer than four live rows, are
left as they are.  Returns a `Warm`: the perturbed CSR batch, its per-instance
densifications and corners in lsap_sparse_families.Batch's form, and the state
(col0 int32 [B, nr], v0 float64 [B, nc]).
"""
from __future__ import annotations

import collections
import functools
import hashlib

import numpy as np

import lsap_sparse_families as S

Warm = collections.namedtuple("Warm", "batch col0 v0 changed")

cases = S.cases


def _rng(family, nr, nc, k):
    h = hashlib.sha256(f"warm_sparse:{family}:{nr}:{nc}:{k}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


@functools.lru_cache(maxsize=None)
def state(family, nr, nc):
    """(col0 int32 [B, nr], v0 float64 [B, nc]): the cold solution of the
    unperturbed batch."""
    col, _, v = S.expected(family, nr, nc)
    return col.astype(np.int32), v.astype(np.float64)


def _stored(b, k, nr, nc):
    """(P bool [nr, nc], V float64 [nr, nc]) of instance k of a batch: the
    pattern and the stored values (0 where nothing is stored)."""
    lo, hi = b.indptr[k * nr], b.indptr[(k + 1) * nr]
    rows = np.repeat(np.arange(nr), np.diff(b.indptr[k * nr:(k + 1) * nr + 1]))
    P = np.zeros((nr, nc), dtype=bool)
    V = np.zeros((nr, nc))
    P[rows, b.indices[lo:hi]] = True
    V[rows, b.indices[lo:hi]] = b.data[lo:hi]
    return P, V


def _perturb(P, V, col, corner, rng):
    """Changes (a) - (d) in place; returns the rows changed, in that order (-1: left out)."""
    nrb, ncb = corner
    order = [int(i) for i in rng.permutation(nrb)]
    ia, ic = order[0], order[1]
    rest = order[2:]
    V[ia, col[ia]] += 37                                                    # (a)
    ib = next((i for i in rest if (P[i, :ncb].sum() - 1) > 0), -1)          # (b)
    if ib >= 0:
        free = np.flatnonzero(P[ib, :ncb] & (np.arange(ncb) != col[ib]))
        j = int(free[rng.integers(free.size)])
        live = P[ib, :ncb] & np.isfinite(V[ib, :ncb])
        V[ib, j] = V[ib, :ncb][live].min() - 1
        rest.remove(ib)
    P[ic, col[ic]] = False                                                  # (c)
    V[ic, col[ic]] = 0
    idd = next((i for i in rest if not P[i, :ncb].all()), -1)               # (d)
    if idd >= 0:
        gaps = np.flatnonzero(~P[idd, :ncb])
        j = int(gaps[rng.integers(gaps.size)])
        P[idd, j] = True
        V[idd, j] = 0
    return ia, ib, ic, idd


@functools.lru_cache(maxsize=None)
def perturbed(family, nr, nc):
    b = S.batch(family, nr, nc)
    col0, v0 = state(family, nr, nc)
    parts, dense, changed = [], [], []
    for k in range(len(b.dense)):
        P, V = _stored(b, k, nr, nc)
        corner = b.corners[k] if b.corners is not None else (nr, nc)
        rows = None
        if b.feasible[k] and corner[0] >= 4:
            rows = _perturb(P, V, col0[k].astype(np.int64), corner, _rng(family, nr, nc, k))
        changed.append(rows)
        parts.append(S.csr_of(P, V))
        dense.append(np.where(P, V, np.inf)[:corner[0], :corner[1]])
    base = np.concatenate([[0], np.cumsum([p[1].size for p in parts])])
    indptr = np.concatenate([[0]] + [p[0][1:] + base[k] for k, p in enumerate(parts)]).astype(np.int64)
    pb = S.Batch(indptr, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), dense,
                 None, b.corners)
    return Warm(pb, col0, v0, changed)


def shapes_of(b, nr, nc):
    """int32 [B, 2] for `shapes`, or None for a batch that is not ragged."""
    return None if b.corners is None else np.asarray(b.corners, dtype=np.int32)
