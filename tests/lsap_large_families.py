"""TEST INFRASTRUCTURE ONLY: cost-matrix families and the case list for the
batched LSAP solvers above 1024 columns (santa_hip.solve_batched_large), in the
style of lsap_families.py and reusing its generators.

Above 1024 columns the integer solver packs its step key with 12-bit fields
(sap_solve_mw, FB = 12): LOB = 25 low bits, BIAS = 2^38, so a step whose
winner's d = spc - minVal_prev lies outside [WINDOW_LO12, WINDOW_HI12) =
[2^32 - 2^38, 2^38 - 2^32) is re-decided by the exact two-pass argmin.  The
families put steps on, next to and far outside both edges, and `tiny_range`
makes nearly every step a tie, so a position, row or column field that kept
10 bits shows as soon as rows and columns pass 1023.

Every generator is a pure function of (nr, nc, seed); numpy and torch on the
CPU only.  tests/golden/lsap_large_cases.npz holds scipy's answers and a
sha256 of instance 0 of every case of fixture_cases() (the matrices are rebuilt
from here); tests/golden/lsap_large_replay.npz the replays (col, u, v) that
are too long to repeat in a test.
"""
from __future__ import annotations

import numpy as np
import torch

import lsap_families as F

KEY_FB12 = 12
KEY_LOB12 = 2 * KEY_FB12 + 1
KEY_BIAS12 = 1 << (63 - KEY_LOB12)
WINDOW_LO12 = (1 << 32) - KEY_BIAS12                          # 2^32 - 2^38
WINDOW_HI12 = (1 << (64 - KEY_LOB12)) - (1 << 32) - KEY_BIAS12  # 2^38 - 2^32
EDGE_OFFSETS12 = (WINDOW_HI12 - 1, WINDOW_HI12, WINDOW_HI12 + 1, WINDOW_LO12 - 1, WINDOW_LO12, WINDOW_LO12 + 1, 0)
assert (WINDOW_LO12, WINDOW_HI12) == ((1 << 32) - (1 << 38), (1 << 38) - (1 << 32))


def window_edges12(nr, nc, seed=0):
    """Row i has minimum EDGE_OFFSETS12[i % 7]: the first step of its Dijkstra
    wins with d on, next to, or away from an edge of the 12-bit key's window."""
    rng = F._rng(205, nr, nc, seed)
    C = rng.integers(0, 1 << 16, size=(nr, nc), dtype=np.int64)
    C -= C.min(axis=1, keepdims=True)
    return C + np.array(EDGE_OFFSETS12, dtype=np.int64)[np.arange(nr) % 7][:, None]


def tiny_range(nr, nc, seed=0):
    """Uniform integers in 0..3: nearly every step is a tie, decided by the
    key's position, row and column fields alone."""
    return F._rng(206, nr, nc, seed).integers(0, 4, size=(nr, nc), dtype=np.int64)


def tiny_range_f(nr, nc, seed=0):
    return tiny_range(nr, nc, seed).astype(np.float64)


def inf_band(nr, nc, seed=0):
    """Integers in 0..63 as floats with +inf in four entries of ten; the
    diagonal stays finite, so the instance is feasible.  Exact in float16 and
    bfloat16 too."""
    rng = F._rng(207, nr, nc, seed)
    C = rng.integers(0, 64, size=(nr, nc)).astype(np.float64)
    hole = rng.random((nr, nc)) < 0.4
    hole[np.arange(nr), np.arange(nr)] = False
    C[hole] = np.inf
    return C


def inf_row(nr, nc, seed=0):
    """inf_band with one row of +inf only: infeasible."""
    C = inf_band(nr, nc, seed)
    C[(7 * (seed + 1)) % nr, :] = np.inf
    return C


INT_FAMILIES = {
    "mw": F.mw, "mw_ties": F.mw_ties,
    "two_scale38": F.two_scale(1 << 38, 238), "two_scale39": F.two_scale(1 << 39, 239),
    "two_scale41": F.two_scale(1 << 41, 241),
    "neg_cols": F.neg_cols, "window_edges12": window_edges12, "i32_extremes": F.i32_extremes,
    "tiny_range": tiny_range,
}
INT32_FAMILIES = ("mw", "i32_extremes", "tiny_range")  # fit int32 at every shape below
F64_FAMILIES = {"mw_tenths": F.mw_tenths, "tiny_range": tiny_range_f, "inf_band": inf_band, "inf_row": inf_row}
SEEDLESS = ("mw", "mw_ties", "mw_tenths")

# --------------------------------------------------------------------------- shapes and cases
# wide and cheap, crossing the launch table's edges (2048 | 2049, 3072 | 3073)
WIDE = ((300, 2048), (300, 2049), (300, 3072), (300, 3073), (300, 4096))
PAST = (1000, 1025)     # one past the old limit, most column slots dead
SQUARES = ((1025, 1025), (2049, 2049), (4096, 4096))


def batch_size(nr, nc):
    return 1 if nr == 4096 else 2 if nr >= 1025 else 3


def int_cases():
    """(family, nr, nc) of the integer cases."""
    out = [("mw", nr, nc) for nr, nc in WIDE + (PAST, (1025, 1025))]
    for f in ("window_edges12", "two_scale38", "two_scale39", "two_scale41", "neg_cols", "i32_extremes"):
        out += [(f, nr, nc) for nr, nc in WIDE + (PAST, (1025, 1025))]
    out += [("tiny_range", 2049, 2049), ("tiny_range", 4096, 4096)]
    return out


def float_cases():
    """(family, nr, nc) of the feasible float cases."""
    out = [("mw_tenths", nr, nc) for nr, nc in WIDE + (PAST, (1025, 1025))]
    out += [("tiny_range", 2049, 2049), ("tiny_range", 4096, 4096)]
    out += [("inf_band", nr, nc) for nr, nc in WIDE + (PAST, (1025, 1025))]
    return out


INFEASIBLE_CASE = ("inf_row", 300, 2049)
FRONT_END_CASES = (("rand_f64", "float64", 2000, 2000), ("rand_int", "int64", 2000, 2000))


def rand_f64(nr, nc, seed=0):
    return F._rng(208, nr, nc, seed).random((nr, nc))


def rand_int(nr, nc, seed=0):
    return F._rng(209, nr, nc, seed).integers(0, 1 << 20, size=(nr, nc), dtype=np.int64)


def make(family, dtype, nr, nc, seed=0):
    if family == "rand_f64":
        return rand_f64(nr, nc, seed)
    if family == "rand_int":
        return rand_int(nr, nc, seed)
    return (INT_FAMILIES if dtype == "int64" else F64_FAMILIES)[family](nr, nc, seed)


def instance(family, dtype, nr, nc, k):
    """Instance k of a test batch (lsap_families.instance's rule): seed k, or
    for a seedless family the one matrix with its rows in the order
    row_permutation(nr, k).  dtype: "int64" or "float64"."""
    if family in SEEDLESS:
        return np.ascontiguousarray(make(family, dtype, nr, nc, 0)[F.row_permutation(nr, k)])
    return make(family, dtype, nr, nc, k)


def fixture_cases():
    """(family, dtype, nr, nc) of every case with an entry in
    tests/golden/lsap_large_cases.npz, in fixture order."""
    return ([(f, "int64", nr, nc) for f, nr, nc in int_cases()] +
            [(f, "float64", nr, nc) for f, nr, nc in float_cases() + [INFEASIBLE_CASE]] + list(FRONT_END_CASES))


# Replays recorded in tests/golden/lsap_large_replay.npz: the vectorised replay
# of lsap_duals_ref takes these from several seconds to minutes each.
def recorded_replays():
    """(family, dtype, nr, nc, k) of every recorded replay."""
    out = [(f, "float64", nr, nc, k) for f, nr, nc in float_cases() if f == "mw_tenths"
           for k in range(batch_size(nr, nc))]
    out += [("mw", "int64", nr, nc, k) for nr, nc in WIDE for k in range(batch_size(nr, nc))]
    return out


def narrow(C, dt):
    """A float64 matrix as a CPU tensor of a narrow dtype (rounded to nearest)."""
    return torch.from_numpy(np.ascontiguousarray(C)).to(dt)
