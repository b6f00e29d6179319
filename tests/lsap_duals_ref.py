"""TEST INFRASTRUCTURE ONLY: scipy's shortest-augmenting-path run replayed on
the CPU so that it also returns the dual variables it ends with.

`replay(C)` is the vectorised form (one numpy expression per Dijkstra step over
the `remaining` array, in the style of lsap_families.sap_trace), `replay_state`
its loop from any state (the warm start's, lsap_warm_ref); `replay_scalar`
is the plain loop, kept for cross-checking.  replay and replay_scalar take an
int64 or a float64 matrix with nr <= nc and return (col4row [nr], u [nr],
v [nc]) in the matrix's dtype, or raise ValueError for an infeasible (float, +inf) instance.

The relaxation is `minVal + C[i, j] - u[i] - v[j]` evaluated left to right and
the dual update `u += minVal - spc`, `v -= minVal - spc`, which are the IEEE
operations of scipy's loop and of the GPU solvers: float64 duals are expected
to be equal bit for bit.  minVal is the chosen column's own spc (scipy:
lowest = spc[j]), so the sign of a zero is kept too.  Tie rule of the scan:
among the columns at the minimum the last unassigned one in scan order, else
the first.

The longest replays (a Machol-Wien instance with 1024 columns takes the
vectorised form 20 s) are recorded in tests/golden/lsap_duals_replay.npz, with
the sha256 of each matrix; `replay_instance` reads them from there and replays
everything else.  `python tests/lsap_duals_ref.py` rewrites the file.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import lsap_families as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsap_duals_replay.npz")
# (family, dtype, nr, nc, instance): lsap_families.instance's arguments
RECORDED = (("mw", "int64", 1000, 1024, 0), ("mw", "int64", 1000, 1024, 1),
            ("mw_tenths", "float64", 600, 1024, 0), ("mw_sqrt", "float64", 600, 1024, 0))


def _prepare(C):
    C = np.asarray(C)
    if np.issubdtype(C.dtype, np.integer):
        C = np.ascontiguousarray(C, dtype=np.int64)
        inf = np.iinfo(np.int64).max
    else:
        C = np.ascontiguousarray(C, dtype=np.float64)
        inf = np.inf
    nr, nc = C.shape
    assert nr <= nc, "replay solves wide input (transpose a tall matrix)"
    return C, C.dtype.type, inf, nr, nc


def replay_state(C, col4row, row4col, u, v):
    """The loop from a state (col4row [nr], row4col [nc], u [nr], v [nc]; it is
    not modified): one search for every row without a column, rows ascending
    -> (col4row, u, v, searches)."""
    C, T, inf, nr, nc = _prepare(C)
    u, v = np.array(u, dtype=C.dtype), np.array(v, dtype=C.dtype)
    col4row, row4col = np.array(col4row, dtype=np.int64), np.array(row4col, dtype=np.int64)
    path = -np.ones(nc, dtype=np.int64)
    searches = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for cur in range(nr):
            if col4row[cur] >= 0:
                continue
            searches += 1
            remaining = np.arange(nc - 1, -1, -1)
            spc = np.full(nc, inf, dtype=C.dtype)
            SR, SC = [], []
            minVal, i = T(0), cur
            while True:
                SR.append(i)
                r = minVal + C[i, remaining] - u[i] - v[remaining]
                old = spc[remaining]
                upd = r < old
                s = np.where(upd, r, old)
                spc[remaining] = s
                path[remaining[upd]] = i
                lowest = s.min()
                if not lowest < inf:
                    raise ValueError("cost matrix is infeasible")
                at = np.flatnonzero(s == lowest)
                free = at[row4col[remaining[at]] < 0]
                index = free[-1] if free.size else at[0]
                minVal = s[index]
                j = int(remaining[index])
                SC.append(j)
                remaining[index] = remaining[-1]
                remaining = remaining[:-1]
                if row4col[j] < 0:
                    sink = j
                    break
                i = int(row4col[j])
            u[cur] = u[cur] + minVal
            others = np.array(SR[1:], dtype=np.int64)
            u[others] = u[others] + (minVal - spc[col4row[others]])
            SCa = np.array(SC, dtype=np.int64)
            v[SCa] = v[SCa] - (minVal - spc[SCa])
            j = sink
            while True:
                i = int(path[j])
                row4col[j] = i
                col4row[i], j = j, int(col4row[i])
                if i == cur:
                    break
    return col4row, u, v, searches


def replay(C):
    """The whole run: the loop from the empty state -> (col4row, u, v)."""
    C, _, _, nr, nc = _prepare(C)
    return replay_state(C, -np.ones(nr, dtype=np.int64), -np.ones(nc, dtype=np.int64),
                        np.zeros(nr, dtype=C.dtype), np.zeros(nc, dtype=C.dtype))[:3]


def replay_scalar(C):
    C, T, inf, nr, nc = _prepare(C)
    u = [T(0)] * nr
    v = [T(0)] * nc
    path = [-1] * nc
    col4row = [-1] * nr
    row4col = [-1] * nc
    rows = [[T(x) for x in row] for row in C]
    with np.errstate(over="ignore", invalid="ignore"):
        for cur in range(nr):
            remaining = list(range(nc - 1, -1, -1))
            spc = [T(inf)] * nc
            SR, SC = [], []
            minVal, i = T(0), cur
            sink = -1
            while sink < 0:
                SR.append(i)
                lowest, index = T(inf), -1
                ci, ui = rows[i], u[i]
                for it, j in enumerate(remaining):
                    r = minVal + ci[j] - ui - v[j]
                    if r < spc[j]:
                        path[j] = i
                        spc[j] = r
                    if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                        lowest = spc[j]
                        index = it
                minVal = lowest
                if not minVal < inf:
                    raise ValueError("cost matrix is infeasible")
                j = remaining[index]
                if row4col[j] == -1:
                    sink = j
                else:
                    i = row4col[j]
                SC.append(j)
                remaining[index] = remaining[-1]
                remaining.pop()
            u[cur] = u[cur] + minVal
            for i in SR[1:]:
                u[i] = u[i] + (minVal - spc[col4row[i]])
            for j in SC:
                v[j] = v[j] - (minVal - spc[j])
            j = sink
            while True:
                i = path[j]
                row4col[j] = i
                col4row[i], j = j, col4row[i]
                if i == cur:
                    break
    return (np.array(col4row, dtype=np.int64), np.array(u, dtype=C.dtype), np.array(v, dtype=C.dtype))


def invariants(C, col, u, v):
    """The four exact invariants of integer duals (nr <= nc) as a dict of bools,
    in Python integers so that nothing wraps."""
    C = np.asarray(C).astype(object)
    nr, nc = C.shape
    u, v = np.asarray(u).astype(object), np.asarray(v).astype(object)
    slack = C - u[:, None] - v[None, :]
    free = np.ones(nc, dtype=bool)
    free[np.asarray(col)] = False
    chosen = C[np.arange(nr), np.asarray(col)]
    return {
        "feasible": bool((slack >= 0).all()),
        "tight": bool((slack[np.arange(nr), np.asarray(col)] == 0).all()),
        "sign": bool((v <= 0).all() and (v[free] == 0).all()),
        "gap": int(u.sum() + v.sum()) == int(chosen.sum()),
    }


@functools.lru_cache(maxsize=None)
def _recorded():
    z = np.load(GOLDEN, allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    return {tuple(m["key"]): (m["sha"], z[f"col{i}"], z[f"u{i}"], z[f"v{i}"]) for i, m in enumerate(meta)}


@functools.lru_cache(maxsize=None)
def replay_instance(family, dtype, nr, nc, k):
    """replay(lsap_families.instance(family, dtype, nr, nc, k)) -- from the
    recorded file for the cases in RECORDED (the matrix must still hash to
    what was recorded), computed otherwise.  dtype: "int64" or "float64"."""
    C = F.instance(family, dtype, nr, nc, k)
    key = (family, dtype, nr, nc, k)
    if key in RECORDED:
        sha, col, u, v = _recorded()[key]
        assert sha == F.matrix_sha(C), f"{key}: the matrix changed, rewrite {GOLDEN}"
        return col.astype(np.int64), u, v
    return replay(C)


def write_recorded():
    arrays, meta = {}, []
    for i, key in enumerate(RECORDED):
        C = F.instance(*key)
        col, u, v = replay(C)
        arrays[f"col{i}"], arrays[f"u{i}"], arrays[f"v{i}"] = col.astype(np.int16), u, v
        meta.append({"key": list(key), "sha": F.matrix_sha(C)})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(GOLDEN, **arrays)


if __name__ == "__main__":
    write_recorded()
