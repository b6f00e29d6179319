"""TEST INFRASTRUCTURE ONLY: the small sparse (CSR) instances the k-best tests
on the CSR share, each with its densification, and a child's masked CSR
written out by hand.

`family()` is a tuple of `Inst`: a canonical CSR matrix of `shape` = (nr, nc)
(indptr int64, indices int32, data float64), the live `corner` (nr_b, nc_b) of
it, and `dense`, the densification of that corner (the stored values, +inf
elsewhere; a stored +inf is a missing entry).  Values are small integers, so
ties are everywhere and every order of summation gives the same cost.

  tridiagonal n x n, n = 1..5: exactly F(n+1) = 1, 2, 3, 5, 8 perfect matchings
  the upper bidiagonal 4 x 4: exactly one (the diagonal)
  lsap_sparse_families' word_edges, explicit_zero, empty_row and hall, small
  a row with a stored +inf
  24 seeded random patterns, nr in 1..5, nc - nr in 0..2, about half the
      entries stored, costs 0..7
  ragged corners of a 4 x 6 pattern, entries stored beyond the corner (their
      values NaN: never read)

With k = K the family provably holds instances with count == 0 (empty_row,
hall), 0 < count < K (the tridiagonal and bidiagonal ones) and, by the seed,
count == K; test_kbest_sparse_cpu.py asserts all three.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import lsap_sparse_families as S

K = 12

Inst = collections.namedtuple("Inst", "name indptr indices data shape corner dense")


def _inst(name, P, V, corner=None):
    P = np.asarray(P, dtype=bool)
    indptr, indices, data = S.csr_of(P, V)
    nr, nc = corner if corner is not None else P.shape
    dense = np.where(P, np.asarray(V, dtype=np.float64), np.inf)[:nr, :nc]
    dense.setflags(write=False)
    return Inst(name, indptr, indices, data, P.shape, (nr, nc), dense)


def _of(name, g):
    """An instance of lsap_sparse_families."""
    return _inst(name, np.isfinite(g.dense) | False, np.where(np.isfinite(g.dense), g.dense, 0))


def tridiagonal(n):
    i = np.arange(n)
    P = np.abs(i[:, None] - i[None, :]) <= 1
    return _inst(f"tridiagonal{n}", P, (i[:, None] + 2 * i[None, :]) % 3)


def bidiagonal4():
    i = np.arange(4)
    d = i[None, :] - i[:, None]
    return _inst("bidiagonal4", (d == 0) | (d == 1), (i[:, None] * i[None, :]) % 4)


def stored_inf():
    V = np.array([[1.0, np.inf, 2.0, 0.0], [0.0, 3.0, np.inf, 1.0], [2.0, 2.0, 1.0, np.inf]])
    P = np.ones((3, 4), dtype=bool)
    P[0, 3] = P[2, 0] = False
    return _inst("stored_inf", P, V)


def ragged(corner):
    rng = np.random.default_rng([20261021, 7, *corner])
    P = rng.random((4, 6)) < 0.6
    V = rng.integers(0, 8, size=(4, 6)).astype(np.float64)
    outside = np.ones((4, 6), dtype=bool)
    outside[:corner[0], :corner[1]] = False
    V[outside] = np.nan
    return _inst(f"ragged{corner[0]}x{corner[1]}", P, V, corner=corner)


@functools.lru_cache(maxsize=None)
def family():
    out = [tridiagonal(n) for n in range(1, 6)] + [bidiagonal4()]
    out += [_of("word_edges", S.word_edges(4, 6, 0)), _of("word_edges_sq", S.word_edges(5, 5, 1)),
            _of("explicit_zero", S.explicit_zero(5, 6, 0)), _of("empty_row", S.empty_row(4, 5, 0)),
            _of("hall", S.hall(4, 5, 0)), stored_inf()]
    rng = np.random.default_rng(20261022)
    for q in range(24):
        nr = int(rng.integers(1, 6))
        nc = nr + int(rng.integers(0, 3))
        out.append(_inst(f"random{q}", rng.random((nr, nc)) < 0.5, rng.integers(0, 8, size=(nr, nc))))
    out += [ragged((4, 6)), ragged((3, 4)), ragged((1, 6)), ragged((0, 0)), ragged((2, 2))]
    return tuple(out)


Batch = collections.namedtuple("Batch", "indptr indices data shape shapes dense")


def batch(insts, NR=None, NC=None):
    """The instances as one CSR matrix of B * NR rows over NC columns (each in
    the top-left of its block, the rows below it empty), ragged by `shapes`
    int32 [B, 2]; dense is the padded [B, NR, NC] densification of the STORED
    pattern (entries beyond a corner included: the shapes hide them)."""
    NR = NR or max(g.shape[0] for g in insts)
    NC = NC or max(g.shape[1] for g in insts)
    counts, idx, val = [], [], []
    dense = np.full((len(insts), NR, NC), np.inf)
    for b, g in enumerate(insts):
        c = np.zeros(NR, dtype=np.int64)
        c[:g.shape[0]] = np.diff(g.indptr)
        counts.append(c)
        idx.append(g.indices)
        val.append(g.data)
        rows = np.repeat(np.arange(g.shape[0]), np.diff(g.indptr))
        dense[b, rows, g.indices] = g.data
    indptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    shapes = np.array([g.corner for g in insts], dtype=np.int32)
    return Batch(indptr, np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float64),
                 (len(insts), NR, NC), shapes, dense)


def masked_csr(indptr, indices, data, col, t, Ft):
    """The CSR of M_t, written out entry by entry from the CSR of one instance
    (nr rows): a row i < t keeps its entry on col[i] alone, a row i >= t loses
    the columns col[0 .. t-1], row t also those of Ft (bool over the columns)."""
    nr = len(indptr) - 1
    closed = {int(col[i]) for i in range(t)}
    counts, idx, val = np.zeros(nr, dtype=np.int64), [], []
    for i in range(nr):
        for e in range(int(indptr[i]), int(indptr[i + 1])):
            j = int(indices[e])
            if i < t:
                keep = j == int(col[i])
            else:
                keep = j not in closed and not (i == t and j < len(Ft) and Ft[j])
            if keep:
                counts[i] += 1
                idx.append(j)
                val.append(data[e])
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.asarray(idx, dtype=np.int32),
            np.asarray(val, dtype=np.float64))
