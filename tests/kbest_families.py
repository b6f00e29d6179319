"""TEST INFRASTRUCTURE ONLY: the small instances the k-best tests share, and
brute force over them.

`small_family()` is 60 seeded instances, nr in 1..5, nc - nr in 0..2, with
integer-valued float64 costs in 0..7 (heavy ties); every third one has 35 % of
its entries +inf.  The seed is fixed: the family holds instances with fewer
than 40 finite assignments and instances without any (tests assert both).
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

K_SMALL = 40


@functools.lru_cache(maxsize=None)
def small_family():
    rng = np.random.default_rng(20261021)
    out = []
    for q in range(60):
        nr = int(rng.integers(1, 6))
        nc = nr + int(rng.integers(0, 3))
        C = rng.integers(0, 8, size=(nr, nc)).astype(np.float64)
        if q % 3 == 2:
            C[rng.random((nr, nc)) < 0.35] = np.inf
        C.setflags(write=False)
        out.append(C)
    return tuple(out)


def brute_force(C):
    """The costs of all finite assignments of C (nr <= nc), sorted."""
    nr, nc = C.shape
    rows = np.arange(nr)
    costs = [C[rows, list(perm)].sum() for perm in itertools.permutations(range(nc), nr)]
    return np.sort(np.array([c for c in costs if c < np.inf], dtype=np.float64))


def check_assignments(C, cols, costs, count):
    """cols[:count] are valid, distinct, cost what costs says; the rest is -1 / +inf."""
    nr, nc = C.shape
    seen = set()
    for r in range(count):
        col = cols[r]
        assert ((col >= 0) & (col < nc)).all() and len(set(col.tolist())) == nr, (r, col)
        assert C[np.arange(nr), col].sum() == costs[r] and costs[r] < np.inf
        seen.add(tuple(col.tolist()))
    assert len(seen) == count
    assert (cols[count:] == -1).all() and (costs[count:] == np.inf).all()
