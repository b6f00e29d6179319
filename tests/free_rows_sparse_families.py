"""TEST INFRASTRUCTURE ONLY: small sparse (CSR) instances for free rows on the
CSR, each with its densification, and the previous states they
are re-solved from.

An instance is kbest_sparse_families.Inst: a canonical CSR of `shape`, the live
`corner` of it and `dense`, the densification of that corner (the stored
values, +inf elsewhere).  Values are small integers, so every sum is exact.

`small()` is kbest_sparse_families.family(): tridiagonal and bidiagonal
patterns, word edges, explicit zeros, a stored +inf, an empty real row and a
Hall-deficient pair of real rows (both wide: infeasible although the virtual
rows have every column), seeded random patterns, and ragged corners with
entries stored beyond them.

`special()` adds what only this mode can get wrong:

  empty_word_mid    20 x 150: no real row stores a column of word 1 (64..127),
                    so only virtual rows can take those; row 0 stores nothing
                    but two columns of the last partial word; nc - nr > 64
  empty_word_last   20 x 150: no real row stores a column of the last partial
                    word (128..149)
  many_virtual      30 x 300: nc - nr = 270 > 256, the virtual rows' rank prefix
                    crosses lanes, waves and rounds
  one_row           1 x 70: nr = 1, entries in both words
  all_and_none      4 x 7: column 2 stored by every real row, column 5 by none;
                    explicit zeros and a stored +inf
  hall_wide         3 x 9: rows 0 and 1 store column 4 alone

`states(inst, seed)` yields (name, col0 int32 [nr], v0 float64 [nc]) over the
instance's whole (unclipped) shape: the cold solution where there is one
("solved"), that with one row pointing at a column it does not store
("dropped"), garbage, and the empty state.
"""
from __future__ import annotations

import functools

import numpy as np

import kbest_sparse_families as KS
import lsap_duals_ref as R

Inst = KS.Inst
batch = KS.batch
small = KS.family


def _seeded(name, nr, nc, keep, seed):
    """The diagonal plus seeded random entries, restricted by keep(P)."""
    rng = np.random.default_rng([20261021, 23, seed])
    P = rng.random((nr, nc)) < 0.15
    P[np.arange(nr), np.arange(nr)] = True
    P = keep(P)
    return KS._inst(name, P, rng.integers(0, 50, size=(nr, nc)))


def empty_word_mid():
    def keep(P):
        P[:, 64:128] = False
        P[0] = False
        P[0, [130, 140]] = True
        return P
    return _seeded("empty_word_mid", 20, 150, keep, 0)


def empty_word_last():
    def keep(P):
        P[:, 128:] = False
        return P
    return _seeded("empty_word_last", 20, 150, keep, 1)


def many_virtual():
    return _seeded("many_virtual", 30, 300, lambda P: P, 2)


def one_row():
    P = np.zeros((1, 70), dtype=bool)
    P[0, [3, 63, 64, 69]] = True
    V = np.zeros((1, 70))
    V[0, [3, 63, 64, 69]] = [5, 2, 2, 7]
    return KS._inst("one_row", P, V)


def all_and_none():
    P = np.array([[1, 0, 1, 1, 0, 0, 1],
                  [0, 1, 1, 0, 1, 0, 0],
                  [1, 1, 1, 0, 0, 0, 1],
                  [0, 0, 1, 1, 1, 0, 1]], dtype=bool)
    V = np.array([[0, 9, 3, np.inf, 9, 9, 2],
                  [9, 0, 1, 9, 4, 9, 9],
                  [2, 0, 0, 9, 9, 9, 5],
                  [9, 9, 2, 1, np.inf, 9, 0]])
    return KS._inst("all_and_none", P, V)


def hall_wide():
    P = np.zeros((3, 9), dtype=bool)
    P[0, 4] = P[1, 4] = True
    P[2, [0, 4, 8]] = True
    return KS._inst("hall_wide", P, np.arange(27).reshape(3, 9) % 5)


@functools.lru_cache(maxsize=None)
def special():
    return (empty_word_mid(), empty_word_last(), many_virtual(), one_row(), all_and_none(), hall_wide())


def family():
    return small() + special()


def diag_random(nr, nc, seed, density=0.05, shift=False):
    """The diagonal plus random entries at about `density`: (indptr, indices,
    data float64) of one nr x nc instance with integer values below 1000.
    shift: also the entries (i, (i + 1) % nc), a second perfect matching of the
    rows that shares no pair with the diagonal, so that whatever column row 0
    holds, an assignment without that pair exists."""
    rng = np.random.default_rng([20261021, 29, nr, nc, seed])
    P = rng.random((nr, nc)) < density
    P[np.arange(nr), np.arange(nr)] = True
    if shift:
        P[np.arange(nr), (np.arange(nr) + 1) % nc] = True
    indptr = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(P.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(P)[1].astype(np.int32), rng.integers(0, 1000, size=int(P.sum())).astype(np.float64)


def feasible(g: Inst) -> bool:
    try:
        R.replay(np.asarray(g.dense))
        return g.dense.shape[0] > 0
    except ValueError:
        return False


def states(g: Inst, seed=0):
    nr, nc = g.shape
    nrb, ncb = g.corner
    rng = np.random.default_rng([20261021, 31, seed, nr, nc])
    if nrb > 0 and feasible(g):
        col, _, v = R.replay(np.asarray(g.dense))
        col0 = -np.ones(nr, dtype=np.int32)
        col0[:nrb] = col
        v0 = np.zeros(nc)
        v0[:ncb] = v
        yield "solved", col0, v0
        # a previous col that names a column the row no longer stores
        i = int(rng.integers(nrb))
        gone = np.flatnonzero(~np.isfinite(g.dense[i]))
        if gone.size:
            col1 = col0.copy()
            col1[i] = gone[rng.integers(gone.size)]
            yield "dropped", col1, v0
    yield "garbage", rng.integers(-3, nc + 3, size=nr).astype(np.int32), \
        np.where(rng.random(nc) < 0.2, np.nan, rng.integers(-60, 20, size=nc).astype(np.float64))
    yield "empty", -np.ones(nr, dtype=np.int32), np.zeros(nc)
