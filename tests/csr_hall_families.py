"""TEST INFRASTRUCTURE ONLY: sparsity patterns for the maximum-cardinality
matching of the sparse (CSR) entries and its Hall-violator proof, beside those
of lsap_sparse_families.

Every generator is a pure function of (nr, nc, seed), nr <= nc, and returns an
lsap_sparse_families.Inst (canonical CSR, the densification, `feasible`: whether
the EDGES -- stored entries that are not +inf -- hold a perfect matching of the
rows).  Values are small integers, as there.

  chain_open    rows i < nr - 1 hold {i, i + 1}, row nr - 1 holds {0}: feasible;
                a search that takes the lowest free column gives row i column i,
                so the last search walks the whole chain: nr steps, nr hops
  chain_closed  the same with row nr - 2 cut to {nr - 2}: nr rows on nr - 1
                columns, card == nr - 1, the witness is every row and
                nN == nr - 1 (needs nr >= 2)
  deficient_k   k + d rows are confined to k columns (d in 2..4 by the seed, as
                far as the rows allow), beside a banded rest (needs nr >= 3)
  inf_edges     the stored pattern has a perfect matching, the edges do not:
                two rows (one when nr == 1) keep one finite entry, in a shared
                column, and their own diagonal entries are stored as +inf
  last_word     up to three rows whose entries lie only at the first and the
                last live bit of the last 64-column word (bits 0 and 63 when
                nc is a multiple of 64), beside a banded rest

`cases()` lists (family, nr, nc) over the seams SHAPES (one word / two, the
last word's edge, more rows than a wave has lanes, 64 words), the chains also
at (1025, 1025).  `batch()` stacks lsap_sparse_families.batch_size(nc)
instances (seeds 0..) into one CSR matrix, as there.
"""
from __future__ import annotations

import functools

import numpy as np

import lsap_sparse_families as S
from lsap_sparse_families import Batch, _diag, _inst, _rng

SHAPES = ((1, 1), (3, 5), (64, 64), (63, 65), (40, 129), (300, 300), (60, 1025), (40, 4096))
CHAIN_LARGE = (1025, 1025)
MIN_ROWS = {"chain_closed": 2, "deficient_k": 3}


def _values(tag, nr, nc, seed):
    return _rng(tag, nr, nc, seed).integers(0, 64, size=(nr, nc))


def _chain(nr, nc):
    P = np.zeros((nr, nc), dtype=bool)
    i = np.arange(nr - 1)
    P[i, i] = P[i, i + 1] = True
    P[nr - 1, 0] = True
    return P


def chain_open(nr, nc, seed=0):
    return _inst(_chain(nr, nc), _values("chain_open", nr, nc, seed))


def chain_closed(nr, nc, seed=0):
    assert nr >= 2
    P = _chain(nr, nc)
    P[nr - 2] = False
    P[nr - 2, nr - 2] = True
    return _inst(P, _values("chain_closed", nr, nc, seed), feasible=False)


def _banded(tag, nr, nc, seed):
    rng = _rng(tag, nr, nc, seed)
    return rng, _diag(nr, nc) | (rng.random((nr, nc)) < 3.0 / nc)


def deficient_k(nr, nc, seed=0):
    assert nr >= 3
    rng, P = _banded("deficient_k", nr, nc, seed)
    d = min(2 + seed % 3, nr - 1)
    k = min(5, nr - d)
    rows = rng.choice(nr, size=k + d, replace=False)
    cols = rng.choice(nc, size=k, replace=False)
    for i in rows:
        P[i] = False
        keep = rng.random(k) < 0.6
        keep[rng.integers(k)] = True
        P[i, cols[keep]] = True
    return _inst(P, _values("deficient_k", nr, nc, seed), feasible=False)


def inf_edges(nr, nc, seed=0):
    rng, P = _banded("inf_edges", nr, nc, seed)
    V = rng.integers(0, 64, size=(nr, nc)).astype(np.float64)
    rows = sorted({nr // 3, nr - 1})
    c = (seed * 37 + nc - 1) % nc
    for i in rows:
        P[i] = False
        P[i, i] = True
        V[i, i] = np.inf
    if nr > 1:  # (a single row keeps its +inf diagonal alone)
        for i in rows:
            P[i, c] = True
            V[i, c] = 5.0
    return _inst(P, V, feasible=False)


def last_word(nr, nc, seed=0):
    rng, P = _banded("last_word", nr, nc, seed)
    cols = sorted({64 * ((nc - 1) // 64), nc - 1})
    rows = rng.choice(nr, size=min(3, nr), replace=False)
    for i in rows:
        P[i] = False
        P[i, cols] = True
    return _inst(P, _values("last_word", nr, nc, seed), feasible=None)  # (ask the reference)


FAMILIES = {"chain_open": chain_open, "chain_closed": chain_closed, "deficient_k": deficient_k,
            "inf_edges": inf_edges, "last_word": last_word}


def cases():
    out = [(f, nr, nc) for f in FAMILIES for nr, nc in SHAPES if nr >= MIN_ROWS.get(f, 1)]
    return out + [("chain_open",) + CHAIN_LARGE, ("chain_closed",) + CHAIN_LARGE]


def all_cases():
    """cases() and those of lsap_sparse_families at the same seams, each as
    (module, family, nr, nc)."""
    mine = [(__name__, f, nr, nc) for f, nr, nc in cases()]
    return mine + [(S.__name__, f, nr, nc) for f, nr, nc in S.cases() if (nr, nc) in SHAPES]


@functools.lru_cache(maxsize=None)
def instance(family, nr, nc, seed):
    return FAMILIES[family](nr, nc, seed)


@functools.lru_cache(maxsize=None)
def batch(family, nr, nc):
    """lsap_sparse_families.batch for these families (corners: None)."""
    insts = [instance(family, nr, nc, k) for k in range(S.batch_size(nc))]
    base = np.concatenate([[0], np.cumsum([g.indices.size for g in insts])])
    indptr = np.concatenate([[0]] + [g.indptr[1:] + base[k] for k, g in enumerate(insts)]).astype(np.int64)
    return Batch(indptr, np.concatenate([g.indices for g in insts]), np.concatenate([g.data for g in insts]),
                 [g.dense for g in insts], [g.feasible for g in insts], None)


def batch_of(module, family, nr, nc):
    return (batch if module == __name__ else S.batch)(family, nr, nc)
