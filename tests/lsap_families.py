"""TEST INFRASTRUCTURE ONLY: deterministic cost-matrix families for the batched
LSAP solvers, and a tracer of scipy's shortest-augmenting-path run.

Random noise leaves most of a SAP kernel idle: a Dijkstra ends after a dozen
steps, an augmenting path has a few hops, and every value sits far inside (or,
scaled up, far outside) the packed key's window.  The families here are built
to reach what noise does not:

* `mw*`: the Machol-Wien instance C[i][j] = (i+1)(j+1) and relatives: about
  nr / 2 Dijkstra steps per row and a last augmenting path of nr hops;
* `two_scale*`, `neg_cols`, `window_edges`: integer values that put single
  steps of a solve outside the window [WINDOW_LO, WINDOW_HI) of the packed
  step key of sap_solve_mw (the step is then re-decided by the exact two-pass
  argmin), above it, below it, and exactly on either edge;
* `i32_extremes`, `mw_neg`: negative values and both ends of int32;
* the float64 and narrow-dtype families: subnormals, a dtype's largest finite
  value with either sign, sums that overflow to +inf, and 600 decades.

Every generator is a pure function of (nr, nc, seed); numpy and torch on the
CPU only, no GPU call.  tests/golden/lsap_adversarial_cases.npz holds scipy's
answers and a sha256 of each matrix (the matrices are rebuilt from here).
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

# The packed step key of sap_solve_mw (csrc/santa_hip.hip, FB = 10): LOB =
# 2 FB + 1 = 21 low bits, BIAS = 2^(63 - LOB) = 2^42; a step whose winner's
# d = spc - minVal_prev has sb = d + BIAS outside [2^32, 2^(64 - LOB) - 2^32)
# is re-decided exactly.  So the window of d is [WINDOW_LO, WINDOW_HI).
KEY_FB = 10
KEY_LOB = 2 * KEY_FB + 1
KEY_BIAS = 1 << (63 - KEY_LOB)
WINDOW_LO = (1 << 32) - KEY_BIAS                      # 2^32 - 2^42
WINDOW_HI = (1 << (64 - KEY_LOB)) - (1 << 32) - KEY_BIAS  # 2^42 - 2^32
EDGE_OFFSETS = (WINDOW_HI - 1, WINDOW_HI, WINDOW_HI + 1, WINDOW_LO - 1, WINDOW_LO, WINDOW_LO + 1, 0)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I32_SPECIALS = (I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX)
DBL_MAX = float(np.finfo(np.float64).max)
# 10^k, k = -300 .. 299, each correctly rounded (parsed, not computed with pow)
POW10 = np.array([float(f"1e{k}") for k in range(-300, 300)])

NARROW = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _rng(tag, nr, nc, seed):
    return np.random.default_rng([20250607, tag, nr, nc, seed])


def _mw(nr, nc):
    i, j = np.indices((nr, nc))
    return (i + 1) * (j + 1)


# --------------------------------------------------------------------------- integer families (int64)
def mw(nr, nc, seed=0):
    return _mw(nr, nc).astype(np.int64)


def mw_neg(nr, nc, seed=0):
    i, j = np.indices((nr, nc))
    return (-((nr - i) * (nc - j))).astype(np.int64)


def mw_ties(nr, nc, seed=0):
    return (_mw(nr, nc) // 64).astype(np.int64)


def two_scale(big, tag):
    def gen(nr, nc, seed=0, g=5):
        """Noise below 2^16; in every other group of g rows all but g - 1
        "cheap" columns carry `big` more: the group's g rows compete for g - 1
        cheap columns, so single steps of a solve cross the scale gap."""
        rng = _rng(tag, nr, nc, seed)
        C = rng.integers(0, 1 << 16, size=(nr, nc), dtype=np.int64)
        for s in range(0, nr, 2 * g):
            cheap = rng.choice(nc, size=g - 1, replace=False)
            add = np.full(nc, big, dtype=np.int64)
            add[cheap] = 0
            C[s:s + g] += add
        return C
    return gen


def neg_cols(nr, nc, seed=0):
    rng = _rng(4, nr, nc, seed)
    C = rng.integers(0, 1 << 16, size=(nr, nc), dtype=np.int64)
    C[:, ::3] -= 1 << 44
    return C


def window_edges(nr, nc, seed=0):
    """Row i has minimum EDGE_OFFSETS[i % 7]: the first step of its Dijkstra
    wins with d on, next to, or away from an edge of the key's window."""
    rng = _rng(5, nr, nc, seed)
    C = rng.integers(0, 1 << 16, size=(nr, nc), dtype=np.int64)
    C -= C.min(axis=1, keepdims=True)
    return C + np.array(EDGE_OFFSETS, dtype=np.int64)[np.arange(nr) % 7][:, None]


def i32_extremes(nr, nc, seed=0):
    rng = _rng(6, nr, nc, seed)
    C = rng.integers(I32_MIN, I32_MAX + 1, size=(nr, nc), dtype=np.int64)
    special = np.array(I32_SPECIALS, dtype=np.int64)[rng.integers(0, len(I32_SPECIALS), size=(nr, nc))]
    return np.where(rng.random((nr, nc)) < 0.5, C, special)


INT_FAMILIES = {
    "mw": mw, "mw_neg": mw_neg, "mw_ties": mw_ties,
    "two_scale42": two_scale(1 << 42, 142), "two_scale43": two_scale(1 << 43, 143),
    "two_scale45": two_scale(1 << 45, 145),
    "neg_cols": neg_cols, "window_edges": window_edges, "i32_extremes": i32_extremes,
}
INT32_FAMILIES = ("mw", "mw_neg", "mw_ties", "i32_extremes")  # fit int32 (the mw ones up to 1024 columns)
SEEDLESS = ("mw", "mw_neg", "mw_ties", "mw_tenths", "mw_sqrt")


# --------------------------------------------------------------------------- float64 families
def mw_tenths(nr, nc, seed=0):
    return _mw(nr, nc) * 0.1


def mw_sqrt(nr, nc, seed=0):
    return np.sqrt(_mw(nr, nc).astype(np.float64))


def decimal(nr, nc, seed=0):
    return _rng(10, nr, nc, seed).integers(0, 30, size=(nr, nc)) * 0.1


def huge(nr, nc, seed=0):
    return _rng(11, nr, nc, seed).random((nr, nc)) * 1e308


def max_overflow(nr, nc, seed=0):
    rng = _rng(12, nr, nc, seed)
    C = rng.random((nr, nc)) * DBL_MAX
    C[rng.random((nr, nc)) < 0.3] = DBL_MAX
    return C


def neg_max(nr, nc, seed=0):
    rng = _rng(13, nr, nc, seed)
    C = rng.random((nr, nc)) * DBL_MAX
    C[rng.random((nr, nc)) < 0.3] = -DBL_MAX
    return C


def subnormal64(nr, nc, seed=0):
    return _rng(14, nr, nc, seed).integers(0, 9, size=(nr, nc)) * 5e-324


def multiscale(nr, nc, seed=0):
    rng = _rng(15, nr, nc, seed)
    return POW10[rng.integers(-300, 300, size=(nr, nc)) + 300] * rng.standard_normal((nr, nc))


F64_FAMILIES = {
    "mw_tenths": mw_tenths, "mw_sqrt": mw_sqrt, "decimal": decimal, "huge": huge,
    "max_overflow": max_overflow, "neg_max": neg_max, "subnormal64": subnormal64, "multiscale": multiscale,
}


# --------------------------------------------------------------------------- narrow dtypes (CPU tensors)
def smallest_subnormal(dt):
    fi = torch.finfo(dt)
    return fi.smallest_normal * fi.eps  # 2^-149 / 2^-24 / 2^-133, exact in float64


def _is_subnormal(t):
    a = t.double().abs()
    return (a > 0) & (a < torch.finfo(t.dtype).smallest_normal)


def subnormal(dt, tag):
    def gen(nr, nc, seed=0):
        x = _rng(tag, nr, nc, seed).integers(0, 8, size=(nr, nc)) * smallest_subnormal(dt)
        t = torch.from_numpy(x).to(dt)
        assert np.array_equal(t.double().numpy(), x), "the cast must be exact"
        return t
    return gen


def mix_subnormal(dt, tag):
    def gen(nr, nc, seed=0):
        rng = _rng(tag, nr, nc, seed)
        sub = rng.integers(0, 8, size=(nr, nc)) * smallest_subnormal(dt)
        wide = rng.standard_normal((nr, nc)) * 4 * torch.finfo(dt).smallest_normal
        t = torch.from_numpy(np.where(rng.random((nr, nc)) < 0.5, sub, wide)).to(dt)
        assert int(_is_subnormal(t).sum()) > nr * nc // 4, "the matrix must hold nonzero subnormals"
        return t
    return gen


def dtype_max(dt, tag):
    def gen(nr, nc, seed=0):
        fmax = torch.finfo(dt).max
        x = _rng(tag, nr, nc, seed).random((nr, nc)) * fmax
        t = torch.from_numpy(x).to(dt).clamp(-fmax, fmax)  # (a value that rounds up to inf: the maximum)
        t[::7, ::5] = fmax
        t[1::7, ::3] = -fmax
        assert bool(torch.isfinite(t).all())
        return t
    return gen


def mw_sqrt_as(dt):
    def gen(nr, nc, seed=0):
        return torch.from_numpy(mw_sqrt(nr, nc)).to(dt)
    return gen


NARROW_FAMILIES = {}  # (family, dtype name) -> generator
for _k, (_name, _dt) in enumerate(sorted(NARROW.items())):
    NARROW_FAMILIES["subnormal", _name] = subnormal(_dt, 20 + _k)
    NARROW_FAMILIES["mix_subnormal", _name] = mix_subnormal(_dt, 30 + _k)
    NARROW_FAMILIES["dtype_max", _name] = dtype_max(_dt, 40 + _k)
    NARROW_FAMILIES["mw_sqrt", _name] = mw_sqrt_as(_dt)
NARROW_NAMES = ("subnormal", "mix_subnormal", "dtype_max", "mw_sqrt")


# --------------------------------------------------------------------------- one surface for fixtures and tests
def make(family, dtype, nr, nc, seed=0):
    """The matrix of (family, dtype name): a numpy int64 / float64 array, or a
    CPU tensor for a narrow dtype."""
    if dtype == "int64":
        return INT_FAMILIES[family](nr, nc, seed)
    if dtype == "float64":
        return F64_FAMILIES[family](nr, nc, seed)
    return NARROW_FAMILIES[family, dtype](nr, nc, seed)


def all_families():
    """(family, dtype name) of every family, in fixture order."""
    return ([(f, "int64") for f in INT_FAMILIES] + [(f, "float64") for f in F64_FAMILIES] +
            [(f, d) for d in sorted(NARROW) for f in NARROW_NAMES])


def as_float64(C):
    """What scipy solves: the float64 image of a matrix of any family."""
    if isinstance(C, torch.Tensor):
        return C.double().numpy()
    return np.ascontiguousarray(C, dtype=np.float64)


def matrix_sha(C):
    """sha256 of the matrix bytes at its own width (row-major)."""
    if isinstance(C, torch.Tensor):
        C = C.contiguous().view(torch.uint8).numpy()
    return hashlib.sha256(np.ascontiguousarray(C).tobytes()).hexdigest()


def row_permutation(nr, k):
    """Fixed row orders for the seedless mw* families: the identity (k = 0),
    the reversal (k = 1), a stride walk (k >= 2)."""
    if k == 0:
        return np.arange(nr)
    if k == 1:
        return np.arange(nr)[::-1].copy()
    return np.random.default_rng([77, nr, k]).permutation(nr)


def instance(family, dtype, nr, nc, k):
    """Instance k of a test batch: seed k, or for a seedless family the rows
    of the one matrix in the order row_permutation(nr, k).  k = 0 is the
    fixture's matrix."""
    if family in SEEDLESS:
        C = make(family, dtype, nr, nc, 0)
        p = row_permutation(nr, k)
        return C[torch.from_numpy(p)] if isinstance(C, torch.Tensor) else np.ascontiguousarray(C[p])
    return make(family, dtype, nr, nc, k)


# --------------------------------------------------------------------------- tracer
def sap_trace(C):
    """scipy's shortest-augmenting-path run on an int64 matrix (nr <= nc), one
    numpy expression per Dijkstra step over the `remaining` array.  Tie rule
    of the scan: among the columns at the minimum the last unassigned one in
    scan order, else the first.

    Returns (col4row [nr], d [steps], first [steps] bool, longest): d is the
    step's lowest - minVal_prev (the quantity the packed key holds), first
    marks each Dijkstra's first step, longest is the longest augmenting path
    in hops (rows re-assigned)."""
    C = np.ascontiguousarray(C, dtype=np.int64)
    nr, nc = C.shape
    assert nr <= nc
    INF = np.iinfo(np.int64).max
    u = np.zeros(nr, dtype=np.int64)
    v = np.zeros(nc, dtype=np.int64)
    path = -np.ones(nc, dtype=np.int64)
    col4row = -np.ones(nr, dtype=np.int64)
    row4col = -np.ones(nc, dtype=np.int64)
    ds, first = [], []
    longest = 0
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1)
        spc = np.full(nc, INF, dtype=np.int64)
        SR, SC = [], []
        minVal, i = 0, cur
        while True:
            SR.append(i)
            r = minVal + C[i, remaining] - u[i] - v[remaining]
            old = spc[remaining]
            upd = r < old
            s = np.where(upd, r, old)
            spc[remaining] = s
            path[remaining[upd]] = i
            lowest = int(s.min())
            at = np.flatnonzero(s == lowest)
            free = at[row4col[remaining[at]] < 0]
            index = free[-1] if free.size else at[0]
            ds.append(lowest - minVal)
            first.append(len(SR) == 1)
            minVal = lowest
            j = int(remaining[index])
            SC.append(j)
            remaining[index] = remaining[-1]
            remaining = remaining[:-1]
            if row4col[j] < 0:
                sink = j
                break
            i = int(row4col[j])
        u[cur] += minVal
        others = np.array(SR[1:], dtype=np.int64)
        u[others] += minVal - spc[col4row[others]]
        SCa = np.array(SC, dtype=np.int64)
        v[SCa] -= minVal - spc[SCa]
        j, hops = sink, 0
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            hops += 1
            if i == cur:
                break
        longest = max(longest, hops)
    return col4row, np.array(ds, dtype=np.int64), np.array(first, dtype=bool), longest
