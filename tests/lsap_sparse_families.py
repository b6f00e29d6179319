"""TEST INFRASTRUCTURE ONLY: sparse (CSR) input families of the batched LSAP
solver, a missing entry being a forbidden pair.

Every generator is a pure function of (nr, nc, seed), nr <= nc, and returns an
`Inst`: a canonical CSR matrix (indptr int64, indices int32 strictly increasing
inside each row, data float64), its densification (the stored values, +inf
elsewhere), whether a full matching of the rows exists, and -- the `ragged`
family only -- the live corner (nr_b, nc_b) of the padded instance.  Values are
small integers (0..63): exact in float32, and ties are everywhere.  The
feasible families keep their diagonal (or, where a row is confined to the last
64-column word, a second set of distinct columns), so they are feasible by
construction.

  band_3, band_5pct, band_40pct  the diagonal plus random entries (about 3 a
              row, 5 %, 40 %)
  word_edges  entries only in columns that are 0 or 63 mod 64, plus the
              diagonal; some rows whose entries all lie in the last 64-column
              word; some rows with an empty word between two populated ones
  full        every entry stored (the dense solve), a few of them +inf
  explicit_zero  stored 0.0 entries beside missing ones: of every four rows the
              first two hold a stored zero on each other's diagonal column and
              the other two pay at least 1, so reading a stored zero as
              missing, or a missing entry as zero, changes col
  bidiagonal  row i holds columns i and i + 1; every 24th row is dear on its
              way forward, so its augmentation walks back the whole run of rows
              that were shifted one column right (a square instance's last row
              walks back the rest)
  empty_row   band_5pct with one row emptied: infeasible
  hall        band_5pct with two rows whose only entry is the same column:
              infeasible (needs two rows: no (1, 1) case)
  uneven      the density goes with the seed, from 40 % over nothing at all
              (seed 1: infeasible) to the bare diagonal, so a batch's indptr
              bases are non-zero and irregular
  ragged      the instance is the corner (nr_b, nc_b) of its padded matrix, by
              the seed (the whole matrix, a proper corner, one row, nothing);
              stored entries outside the corner hold NaN

`cases()` lists (family, nr, nc) over SHAPES, the smallest shapes that cross
each seam of the launch table (one wave / four waves at 64 columns, the 1 / 2 /
4 columns per thread at 256 and 512, eight waves with 4 / 6 / 8 columns above
1024, 2048 and 3072), plus one square (1025, 1025) band_3.  `batch()` stacks
batch_size(nc) instances (seeds 0..) into one CSR matrix of B * nr rows.
"""
from __future__ import annotations

import collections
import functools
import hashlib

import numpy as np

Inst = collections.namedtuple("Inst", "indptr indices data dense feasible corner")
Batch = collections.namedtuple("Batch", "indptr indices data dense feasible corners")

SHAPES = ((1, 1), (3, 5), (64, 64), (63, 65), (40, 129), (100, 257), (100, 513), (300, 300), (60, 1024),
          (60, 1025), (40, 2049), (40, 3073), (40, 4096))
SQUARE_LARGE = ("band_3", 1025, 1025)


def _rng(tag, nr, nc, seed):
    h = hashlib.sha256(f"sparse:{tag}:{nr}:{nc}:{seed}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


def csr_of(P, V):
    """Canonical CSR of the entries of V that P marks as stored."""
    P = np.asarray(P, dtype=bool)
    indptr = np.zeros(P.shape[0] + 1, dtype=np.int64)
    np.cumsum(P.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(P)[1].astype(np.int32), np.asarray(V, dtype=np.float64)[P]


def _inst(P, V, feasible=True, corner=None):
    indptr, indices, data = csr_of(P, V)
    dense = np.where(P, np.asarray(V, dtype=np.float64), np.inf)
    if corner is not None:
        dense = dense[:corner[0], :corner[1]]
    return Inst(indptr, indices, data, dense, feasible, corner)


def _diag(nr, nc):
    P = np.zeros((nr, nc), dtype=bool)
    P[np.arange(nr), np.arange(nr)] = True
    return P


def _band(tag, p):
    def gen(nr, nc, seed=0):
        rng = _rng(tag, nr, nc, seed)
        P = _diag(nr, nc) | (rng.random((nr, nc)) < (p if p < 1 else p / nc))
        return _inst(P, rng.integers(0, 64, size=(nr, nc)))
    return gen


band_3, band_5pct, band_40pct = _band("band_3", 3.0), _band("band_5pct", 0.05), _band("band_40pct", 0.40)


def word_edges(nr, nc, seed=0):
    rng = _rng("word_edges", nr, nc, seed)
    j = np.arange(nc)
    P = _diag(nr, nc) | ((rng.random((nr, nc)) < 0.5) & ((j % 64 == 0) | (j % 64 == 63))[None, :])
    nwords, L0 = (nc + 63) // 64, 64 * ((nc - 1) // 64)
    # rows confined to the last word: rows whose diagonal lies there, or, where
    # no diagonal does, rows 1, 3, 5 with the distinct columns L0, L0 + 1, ..
    if L0 < nr:
        last = [(i, i) for i in range(L0, nr, 2)]
    else:
        last = [(2 * m + 1, L0 + m) for m in range(min(3, nc - L0)) if 2 * m + 1 < nr]
    for i, c in last:
        keep = P[i, L0:] | (rng.random(nc - L0) < 0.3)
        P[i] = False
        P[i, L0:] = keep
        P[i, c] = True
    # rows with an empty word between two populated ones
    confined = {i for i, _ in last}
    for i in range(2, nr, 7):
        if nwords < 3 or i in confined:
            continue
        m = 1 + (i // 7) % (nwords - 2)
        if i // 64 == m:
            continue
        P[i, 64 * m:64 * (m + 1)] = False
        P[i, 64 * (m - 1)] = True
        P[i, 64 * (m + 1)] = True
    return _inst(P, rng.integers(0, 64, size=(nr, nc)))


def full(nr, nc, seed=0):
    rng = _rng("full", nr, nc, seed)
    V = rng.integers(0, 64, size=(nr, nc)).astype(np.float64)
    V[(rng.random((nr, nc)) < 0.03) & ~_diag(nr, nc)] = np.inf
    return _inst(np.ones((nr, nc), dtype=bool), V)


def explicit_zero(nr, nc, seed=0):
    rng = _rng("explicit_zero", nr, nc, seed)
    P = _diag(nr, nc) | (rng.random((nr, nc)) < 0.10)
    V = rng.integers(1, 64, size=(nr, nc))
    V[np.arange(nr), np.arange(nr)] = 10
    for i in range(0, nr - 1, 4):  # the swap of rows i, i + 1 costs 0 against 20; rows i + 2, i + 3 pay
        P[i, i + 1] = P[i + 1, i] = True
        V[i, i + 1] = V[i + 1, i] = 0
    return _inst(P, V)


def bidiagonal(nr, nc, seed=0):
    P = _diag(nr, nc)
    V = np.zeros((nr, nc), dtype=np.int64)
    for i in range(nr):
        V[i, i] = 1 + (i + seed) % 2  # (the seed only varies the ties)
        if i + 1 < nc:
            P[i, i + 1] = True
            V[i, i + 1] = 63 if i % 24 == 23 else 0
    return _inst(P, V)


def empty_row(nr, nc, seed=0):
    g = band_5pct(nr, nc, seed)
    P = np.isfinite(g.dense)
    P[nr // 2] = False
    return _inst(P, np.where(P, g.dense, 0), feasible=False)


def hall(nr, nc, seed=0):
    assert nr >= 2, "two rows share their only column"
    g = band_5pct(nr, nc, seed)
    P = np.isfinite(g.dense)
    a, b = nr // 3, nr - 1
    c = (seed * 37 + nc - 1) % nc
    P[[a, b]] = False
    P[[a, b], c] = True
    return _inst(P, np.where(np.isfinite(g.dense), g.dense, 7), feasible=False)


UNEVEN = (0.40, None, 0.0, 0.02, 0.90, 0.10, 0.0, 0.25)  # None: no entry at all


def uneven(nr, nc, seed=0):
    rng = _rng("uneven", nr, nc, seed)
    p = UNEVEN[seed % len(UNEVEN)]
    if p is None:
        return _inst(np.zeros((nr, nc), dtype=bool), np.zeros((nr, nc)), feasible=False)
    P = _diag(nr, nc) | (rng.random((nr, nc)) < p)
    return _inst(P, rng.integers(0, 64, size=(nr, nc)))


def ragged_corner(nr, nc, seed):
    return ((nr, nc), ((nr + 1) // 2, nc // 2 + 1), (1, nc), (0, 0),
            (max(nr - 1, 0), nc), (nr, max(nc - 1, nr)), (min(nr, 2), nc), (0, nc))[seed % 8]


def ragged(nr, nc, seed=0):
    rng = _rng("ragged", nr, nc, seed)
    nrb, ncb = ragged_corner(nr, nc, seed)
    P = _diag(nr, nc) | (rng.random((nr, nc)) < 0.10)
    V = rng.integers(0, 64, size=(nr, nc)).astype(np.float64)
    outside = np.ones((nr, nc), dtype=bool)
    outside[:nrb, :ncb] = False
    V[outside] = np.nan
    return _inst(P, V, feasible=nrb > 0, corner=(nrb, ncb))


FAMILIES = {"band_3": band_3, "band_5pct": band_5pct, "band_40pct": band_40pct, "word_edges": word_edges,
            "full": full, "explicit_zero": explicit_zero, "bidiagonal": bidiagonal, "empty_row": empty_row,
            "hall": hall, "uneven": uneven, "ragged": ragged}


def cases():
    out = [(f, nr, nc) for f in FAMILIES for nr, nc in SHAPES if not (f == "hall" and nr < 2)]
    return out + [SQUARE_LARGE]


def batch_size(nc):
    return 8 if nc <= 1024 else 2


@functools.lru_cache(maxsize=None)
def instance(family, nr, nc, seed):
    return FAMILIES[family](nr, nc, seed)


@functools.lru_cache(maxsize=None)
def batch(family, nr, nc):
    """The case's batch as one CSR matrix of B * nr rows; dense, feasible and
    corners are per-instance lists (corners None unless the family is ragged)."""
    insts = [instance(family, nr, nc, k) for k in range(batch_size(nc))]
    base = np.concatenate([[0], np.cumsum([g.indices.size for g in insts])])
    indptr = np.concatenate([[0]] + [g.indptr[1:] + base[k] for k, g in enumerate(insts)]).astype(np.int64)
    corners = [g.corner for g in insts] if insts[0].corner is not None else None
    return Batch(indptr, np.concatenate([g.indices for g in insts]), np.concatenate([g.data for g in insts]),
                 [g.dense for g in insts], [g.feasible for g in insts], corners)


@functools.lru_cache(maxsize=None)
def expected(family, nr, nc):
    """What a solve of the case's batch must return, computed once per process
    from the densifications: (col [B, nr] of oracle.lsap, u [B, nr], v [B, nc]
    of lsap_duals_ref.replay); -1 and NaN in the live slots of an infeasible
    instance, -1 and 0 in the padding of a ragged one (and in every slot of an
    empty one)."""
    import lsap_duals_ref as R
    import oracle
    b = batch(family, nr, nc)
    B = len(b.dense)
    col, u, v = -np.ones((B, nr), dtype=np.int64), np.zeros((B, nr)), np.zeros((B, nc))
    for k, D in enumerate(b.dense):
        r, c = D.shape
        if r == 0:
            continue
        try:
            col[k, :r] = oracle.lsap(D)[1]
            rcol, u[k, :r], v[k, :c] = R.replay(D)
            assert np.array_equal(rcol, col[k, :r]), (family, nr, nc, k)
        except ValueError:
            u[k, :r], v[k, :c] = np.nan, np.nan
    return col, u, v


def padded_dense(b: Batch, nr, nc):
    """[B, nr, nc] float64 for the dense solver: each instance's densification
    in its corner, +inf in the padding (never read by a ragged solve)."""
    D = np.full((len(b.dense), nr, nc), np.inf)
    for k, d in enumerate(b.dense):
        D[k, :d.shape[0], :d.shape[1]] = d
    return D
