"""TEST INFRASTRUCTURE ONLY: deterministic cost-matrix families for the batched
bottleneck solver (lbap_kernel), the sibling of lsap_families.

Random integers leave most of lbap_kernel idle: a search ends after a few
steps, a path has a few hops, and lbap_key only ever sees small positive
numbers.  The families here are built to reach what noise does not:

* `chain`: one search of exactly nr steps and one augmenting path of exactly
  nr hops (the bound of the kernel's augment loop), at any size;
* `mw`: lsap_families.mw, searches and paths of more than nr / 2 at 513 and
  1025 rows, with ties nowhere;
* `signed_zeros`: +0.0, -0.0 and one value beyond them: a key that orders -0.0
  below +0.0 returns another assignment;
* `nan_patterns`: +inf and NaN of four payloads (quiet, signalling, sign bit
  set, all ones) as the forbidden pairs around a finite permutation;
* `random_bits`: every entry a uniformly random bit pattern of the dtype: all
  exponents, both signs, subnormals, both infinities and NaN;
* `split_words`: integers and doubles that differ in one half of their bits
  only: a 64-bit compare that looks at one word, or takes the low word as
  signed, returns another assignment;
* `small_ints`: random integers of magnitude <= 128, exact in all six dtypes.

Every generator is a pure function of (nr, nc, k) (k: the member of a batch)
and numpy only.  A matrix is kept as it is stored on the device: numpy's own
dtype, and the uint16 bit patterns for bfloat16 (`store`, `widen`).  The
reference of lbap_ref.py runs on the widened values (int64 / float64), which
is exact for every dtype.  `batch` builds a family's batch with its
references; `config_of` mirrors the launch table.
"""
from __future__ import annotations

import collections
import functools
import os

import numpy as np

import lsap_families
from lbap_ref import lbap_ref

DTYPES = ("i64", "i32", "f64", "f32", "f16", "bf16")
FLOATS = ("f64", "f32", "f16", "bf16")
STORE = {"i64": np.int64, "i32": np.int32, "f64": np.float64, "f32": np.float32, "f16": np.float16,
         "bf16": np.uint16}
UINT = {"i64": np.uint64, "i32": np.uint32, "f64": np.uint64, "f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
# (exponent bits, mantissa bits) of the float dtypes
LAYOUT = {"f64": (11, 52), "f32": (8, 23), "f16": (5, 10), "bf16": (8, 7)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbap_adversarial.npz")

# lbap_solve_ flags of include/santa_hip.h (test_lbap_cpu.py pins them to the header)
SH_FLAG_LBAP_MW, SH_FLAG_LBAP_SW = 131072, 262144


def config_of(nc, B, flags):
    """(NW, K) of the lbap_kernel that a batch of B instances with nc columns
    runs: launch_lbap, lbap_mw_default and pick_k of csrc/santa_api.inc."""
    default_mw = nc > 512 or (nc > 256 and B <= 1024)
    mw = nc > 1024 or (not flags & SH_FLAG_LBAP_SW and (bool(flags & SH_FLAG_LBAP_MW) or default_mw))
    if not mw:
        return 1, next(k for k in (1, 2, 4, 8, 16) if nc <= 64 * k)
    return next(cfg for top, cfg in ((256, (4, 1)), (512, (4, 2)), (1024, (4, 4)), (2048, (8, 4)), (4096, (16, 4)))
                if nc <= top)


def _rng(tag, nr, nc, k):
    return np.random.default_rng([20250915, tag, nr, nc, k])


# --------------------------------------------------------------------------- storage
def store(V, dt):
    """int64 / float64 values as the dtype's storage (bfloat16: its bits, of
    the float32 with the same value; the caller checks exactness by `widen`)."""
    V = np.asarray(V)
    if dt == "bf16":
        return (V.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return V.astype(STORE[dt])


def widen(S, dt):
    """Stored values as the reference reads them: int64, or float64 (exact)."""
    S = np.asarray(S)
    with np.errstate(invalid="ignore"):   # (a signalling NaN widens to a quiet one)
        if dt == "bf16":
            return (S.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return S.astype(np.int64 if dt in ("i64", "i32") else np.float64)


def as_bits(S, dt):
    return np.ascontiguousarray(S).view(UINT[dt])


def from_bits(U, dt):
    U = np.ascontiguousarray(U, dtype=UINT[dt])
    return U if dt == "bf16" else U.view(STORE[dt])


def poison(dt, maximize):
    """What would win if the padding of a ragged batch were read."""
    if dt in ("i64", "i32"):
        ii = np.iinfo(STORE[dt])
        return STORE[dt](ii.max if maximize else ii.min)
    return store(np.array(np.inf if maximize else -np.inf), dt)[()]


# --------------------------------------------------------------------------- families
def chain(nr, nc, k=0, big=100):
    """Row i < nr - 1: 0 at column i, 1 at i + 1, `big` elsewhere; the last row
    0 at column 0 and big + 1 elsewhere.  Rows 0 .. nr - 2 take their zeros at
    once; the last row's search then visits columns 0, 1, .. nr - 1 in turn
    (every step's least column is unique) and its path moves every row one
    column up: steps == hops == nr, col = [1 .. nr - 1, 0], value 1.
    k = 1: the columns rotated by a seeded offset; k = 2: the chain in the
    last nr columns."""
    C = np.full((nr, nc), big, dtype=np.int64)
    i = np.arange(nr - 1)
    C[i, i], C[i, i + 1] = 0, 1
    C[nr - 1] = big + 1
    C[nr - 1, 0] = 0
    if k == 1:
        C = np.roll(C, int(_rng(1, nr, nc, k).integers(1, nc)), axis=1)
    elif k == 2:
        C = np.roll(C, nc - nr, axis=1)
    return C


def mw(nr, nc, k=0):
    """lsap_families.mw; k > 0: its rows in a seeded order."""
    C = lsap_families.mw(nr, nc)
    return C if k == 0 else C[_rng(2, nr, nc, k).permutation(nr)]


def signed_zeros(nr, nc, k=0, maximize=False):
    """+0.0, -0.0 and 1.0 (-1.0 under maximize: the side of zero that loses)
    with probabilities .35, .35, .3."""
    u = _rng(3, nr, nc, k).random((nr, nc))
    return np.where(u < 0.35, 0.0, np.where(u < 0.7, -0.0, -1.0 if maximize else 1.0))


def nan_bits(dt):
    """Four NaN of the dtype: quiet, signalling, quiet with the sign bit, all ones."""
    e, m = LAYOUT[dt]
    expo = ((1 << e) - 1) << m
    return np.array([expo | 1 << (m - 1), expo | 1, 1 << (e + m) | expo | 1 << (m - 1), (1 << (e + m + 1)) - 1],
                    dtype=UINT[dt])


def nan_patterns(dt, nr, nc, k=0, maximize=False, feasible=True):
    """test_lbap_gpu.inf_pattern (about half the entries forbidden around a
    finite random permutation, integers below 128 elsewhere) with a NaN in
    place of about half of the infinities, the four payloads in turn, and the
    best possible cost (-inf; +inf under maximize) on about 1 % of the rest.
    Under maximize the finite values are negated and the forbidden infinity is
    -inf.  Not feasible: one row is NaN throughout, nothing else changes."""
    rng = _rng(4, nr, nc, k)
    V = rng.integers(0, 128, size=(nr, nc)).astype(np.float64)
    keep = rng.random((nr, nc)) < 0.5
    keep[np.arange(nr), rng.permutation(nc)[:nr]] = True
    V[keep & (rng.random((nr, nc)) < 0.01)] = -np.inf
    V[~keep] = np.inf
    nan = ~keep & (rng.random((nr, nc)) < 0.5)
    if not feasible:
        nan[nr // 2] = True
    S = store(-V if maximize else V, dt)
    U = as_bits(S, dt).copy()
    U[nan] = nan_bits(dt)[rng.integers(0, 4, size=(nr, nc))][nan]
    return from_bits(U, dt)


def nan_as_its_bits_order(S, dt, maximize):
    """The widened matrix that a key without the NaN branch would solve: the
    sign-magnitude flip puts a NaN without the sign bit above +inf and one with
    it below -inf, so one of them becomes the best possible cost and the other
    a cost above (below) every finite one, which is not forbidden."""
    W = widen(S, dt)
    neg = (as_bits(S, dt) >> np.array(sum(LAYOUT[dt]), dtype=UINT[dt])).astype(bool)
    top = np.finfo(np.float64).max
    W[np.isnan(W) & neg] = -top if maximize else -np.inf
    W[np.isnan(W) & ~neg] = np.inf if maximize else top
    return W


def is_subnormal(S, dt):
    e, m = LAYOUT[dt]
    U = as_bits(S, dt).astype(np.uint64)
    return ((U >> np.uint64(m)) & np.uint64((1 << e) - 1) == 0) & ((U & np.uint64((1 << m) - 1)) != 0)


def random_bits(dt, nr, nc, k=0):
    """Every entry a uniformly random bit pattern of the dtype: the first
    seeded draw that holds a NaN, a subnormal and a negative value (the
    64-bit dtype needs some thousand entries for the first two)."""
    bits = 8 * np.dtype(UINT[dt]).itemsize
    for s in range(1000):
        rng = _rng(5, nr, nc, 1000 * k + s)
        S = from_bits(rng.integers(0, 1 << bits, size=(nr, nc), dtype=np.uint64, endpoint=False).astype(UINT[dt]), dt)
        W = widen(S, dt)
        if np.isnan(W).any() and is_subnormal(S, dt).any() and (W < 0).any():
            return S
    raise AssertionError("no draw with a NaN, a subnormal and a negative value")


SPLIT_FORMS = ("hi_equal", "lo_equal", "mixed")


def split_words(dt, nr, nc, k=0, form="mixed"):
    """Values that differ in one half of their bits.  int64: (hi << 32) | lo,
    int32 the same at 16 bits a half: `hi_equal` one hi and lo uniform,
    `lo_equal` lo = 0x80000001 (0x8001) and hi in -2 .. 1, `mixed` hi in
    -2 .. 1 and lo uniform.  float64: 1.0 + m 2^-52, m uniform in [0, 2^33):
    one upper word (but its lowest bit), and the order in the lower one."""
    rng = _rng(6, nr, nc, k)
    if dt == "f64":
        m = rng.integers(0, 1 << 33, size=(nr, nc), dtype=np.uint64)
        return (np.array(1.0).view(np.uint64) + m).view(np.float64)
    h = 32 if dt == "i64" else 16
    hi = rng.integers(-2, 2, size=(nr, nc))
    lo = rng.integers(0, 1 << h, size=(nr, nc))
    if form == "hi_equal":
        hi[:] = int(rng.integers(-2, 2))
    elif form == "lo_equal":
        lo[:] = (1 << (h - 1)) | 1
    return ((hi << h) | lo).astype(STORE[dt])


def wrong_compares(C, dt):
    """int64 matrices whose order is that of a two-word compare of C gone
    wrong: the high word alone, the low word alone, the low word as signed."""
    h = 32 if dt == "i64" else 16
    C = C.astype(np.int64)
    hi, lo = C >> h, C & ((1 << h) - 1)
    return {"high word only": hi, "low word only": lo, "low word signed": (hi << h) | (lo ^ (1 << (h - 1)))}


def small_ints(nr, nc, k=0):
    return _rng(7, nr, nc, k).integers(-128, 129, size=(nr, nc))


# --------------------------------------------------------------------------- batches
Case = collections.namedtuple("Case", "family dt nr nc maximize")
Batch = collections.namedtuple("Batch", "C shapes refs")   # C [B, nr, nc] stored; refs: (col [nr], value) each


def case_id(c):
    return f"{c.family}-{c.dt}-{c.nr}x{c.nc}" + ("-max" if c.maximize else "")


def members(family, dt, nr, nc, maximize=False):
    """The stored matrices of a case's batch; one with fewer than nr rows is a
    ragged member (passed through `shapes`)."""
    if family == "chain":
        if nc > 2049:       # one full instance and one that is a row short, its chain in the last columns
            V = [chain(nr, nc), chain(nr - 1, nc, 2)]
        elif nc > 257:
            V = [chain(nr, nc), chain(nr, nc, 1)]
        else:
            V = [chain(nr, nc), chain(nr, nc, 1), chain(nr - 3, nc), chain(nr - 3, nc, 2)]
    elif family == "mw":
        V = [mw(nr, nc, k) for k in range(2 if nc <= 513 else 1)]
    elif family == "signed_zeros":
        V = [signed_zeros(nr, nc, k, maximize) for k in range(3)]
    elif family == "small_ints":
        V = [small_ints(nr, nc, k) for k in range(2)]
    elif family == "nan_patterns":
        return [nan_patterns(dt, nr, nc, k, maximize) for k in range(3)] + \
               [nan_patterns(dt, nr, nc, 0, maximize, feasible=False)]
    elif family == "random_bits":
        return [random_bits(dt, nr, nc, k) for k in range(2)]
    elif family == "split_words":
        if dt == "f64":
            return [split_words(dt, nr, nc, k) for k in range(3)]
        return [split_words(dt, nr, nc, 0, "hi_equal"), split_words(dt, nr, nc, 1, "lo_equal"),
                split_words(dt, nr, nc, 2), split_words(dt, nr, nc, 3)]
    else:
        raise KeyError(family)
    return [store(v, dt) for v in V]


VALUE_FAMILIES = ("chain", "mw", "signed_zeros", "small_ints")  # the same values in every dtype: one reference


@functools.lru_cache(maxsize=None)
def _refs(family, dt, nr, nc, maximize):
    """Per member (col, value, steps, hops) of lbap_ref on the widened values
    (the recorded ones for `mw`: tests/golden/make_lbap_adversarial_golden.py)."""
    if family == "mw":
        z = np.load(GOLDEN)
        return [(z[f"mw_{nr}_{k}_col"].astype(np.int32), z[f"mw_{nr}_{k}_value"][()],
                 int(z[f"mw_{nr}_{k}_steps"]), int(z[f"mw_{nr}_{k}_hops"])) for k in range(2 if nc <= 513 else 1)]
    return [lbap_ref(widen(S, dt), maximize) for S in members(family, dt, nr, nc, maximize)]


def refs(family, dt, nr, nc, maximize=False):
    """(Computed once for all dtypes where the values do not depend on it;
    test_lbap_adversarial_cpu.py checks that each dtype holds them exactly.)"""
    return _refs(family, "f64" if family in VALUE_FAMILIES else dt, nr, nc, maximize)


def batch(case):
    """The case's members padded into one tensor, the padding of a ragged
    member holding what would win if it were read."""
    family, dt, nr, nc, maximize = case
    M = members(family, dt, nr, nc, maximize)
    C = np.empty((len(M), nr, nc), dtype=STORE[dt])
    C[:] = poison(dt, maximize)
    for b, S in enumerate(M):
        C[b, :S.shape[0], :S.shape[1]] = S
    ragged = any(S.shape != (nr, nc) for S in M)
    shapes = np.array([S.shape for S in M], dtype=np.int32) if ragged else None
    R = [(np.concatenate([col, np.full(nr - col.size, -1, dtype=np.int32)]), value)
         for col, value, _, _ in refs(family, dt, nr, nc, maximize)]
    return Batch(C, shapes, R)


# --------------------------------------------------------------------------- the cases of test_lbap_adversarial_gpu.py
def _cases():
    out = []
    for nr, nc in ((64, 64), (65, 65), (257, 257)):
        out += [Case("chain", dt, nr, nc, False) for dt in DTYPES]
    for n in (1024, 1025):
        out += [Case("chain", dt, n, n, False) for dt in ("i32", "i64", "f32", "f16")]
    for n in (2048, 2049):
        out += [Case("chain", dt, n, n, False) for dt in ("i64", "bf16")]
    out += [Case("chain", dt, 4096, 4096, False) for dt in ("i32", "f16")]
    out += [Case("mw", dt, n, n, False) for n in (513, 1025) for dt in ("i64", "f32")]
    small = ((40, 60), (65, 65), (200, 257))
    for maximize in (False, True):
        out += [Case("signed_zeros", dt, nr, nc, maximize) for dt in FLOATS for nr, nc in small]
        out += [Case("nan_patterns", dt, nr, nc, maximize) for dt in FLOATS for nr, nc in ((65, 65), (255, 256))]
        out += [Case("random_bits", dt, nr, nc, maximize) for dt in FLOATS for nr, nc in ((40, 60), (130, 257))]
        out += [Case("split_words", dt, nr, nc, maximize) for dt in ("i64", "f64", "i32") for nr, nc in small]
    # the rest of the 60 kernels: one width for each (NW, K, dtype) that nothing above runs
    out += [Case("small_ints", dt, 200, 256, False) for dt in ("i64", "i32")]      # (1, 4), (4, 1)
    out += [Case("small_ints", dt, 513, 513, False) for dt in ("f64", "bf16")]     # (1, 16), (4, 4)
    out += [Case("chain", "f64", 1025, 1025, False)]                               # (8, 4)
    out += [Case("chain", dt, 2049, 2049, False) for dt in ("f64", "f32")]         # (16, 4)
    return out


CASES = _cases()
