"""TEST INFRASTRUCTURE ONLY: instances for the min-sum certificate
(lsap_cert_kernel, lsap_slack_kernel, lsap_cert_final_kernel) that need no
solver, and the places in them where the pass over the corner could lose an
entry ("The certificate against a host reference").

`certified(dt, nr, nc, seed, variant)` builds (C, col, u, v) optimal by
construction: col from a random permutation, u, v <= 0 with v == 0 on the free
columns, slacks S >= 1 off the assignment and 0 on it, C = u + v + S.  The
certificate of it is (0, 0, 0) with flags 0 whatever its size.  Variants:
  plain       u in [0, 64], v in [-64, 0], S in [0, 64]: every value, and every
              plant down to -128, is an integer of magnitude at most 128, exact
              in all six dtypes (asserted on every matrix returned)
  big         int64: |u|, |v| just below 2^61, every C below it too
  ends        int32: rows near INT32_MAX and rows near INT32_MIN, with one entry
              at each end
  multiscale  float64: magnitudes 1e-300 .. 1e299 as lsap_families.multiscale
              draws them; feasible only up to rounding, so what the
              certificate returns for it is lsap_cert_ref.cert_ref's business
A plant (`plant_value`) lowers ONE entry to u[i] + v[j] - d: the instance's
only negative slack, -d, which a pass that skips (i, j) cannot see.

`geometry` mirrors launch_lsap_check and the first lines of lsap_slack_kernel
and `positions` lists the entries at the edges of that geometry.  Both only
choose where to plant and prove that the case list reaches every class of
launch; no expected value comes from them.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from lbap_families import DTYPES, FLOATS, STORE, store, widen  # noqa: F401
from lsap_families import POW10

I32 = np.iinfo(np.int32)
ITEMSIZE = {"i64": 8, "i32": 4, "f64": 8, "f32": 4, "f16": 2, "bf16": 2}
SEEDS = 3   # distinct matrices in a batch of one shape: instance b is seed b % SEEDS

Instance = collections.namedtuple("Instance", "dt variant S col u v")   # S: the stored matrix [nr, nc]


def _rng(tag, nr, nc, seed):
    return np.random.default_rng([20261020, tag, nr, nc, seed])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def certified(dt, nr, nc, seed=0, variant="plain"):
    """-> Instance; col int64 [nr], u [nr] and v [nc] int64 or float64 (read-only)."""
    assert 1 <= nr <= nc
    rng = _rng(1, nr, nc, seed)
    col = rng.permutation(nc)[:nr].astype(np.int64)
    on = np.zeros((nr, nc), dtype=bool)
    on[np.arange(nr), col] = True
    taken = on.any(axis=0)
    if variant == "multiscale":
        assert dt == "f64"
        mag = lambda n: POW10[rng.integers(-300, 300, size=n) + 300]  # noqa: E731
        u = mag(nr) * rng.standard_normal(nr)
        v = np.where(taken, -np.abs(mag(nc) * rng.standard_normal(nc)), 0.0)
        S = np.where(on, 0.0, np.abs(mag((nr, nc)) * rng.standard_normal((nr, nc))))
        C = u[:, None] + v[None, :] + S
        assert np.isfinite(C).all()
        return Instance(dt, variant, *_frozen(C, col, u, v))
    lim = 64 if variant == "plain" else 32
    u = rng.integers(0, lim + 1, size=nr)
    v = np.where(taken, -rng.integers(0, lim + 1, size=nc), 0)
    S = np.where(on, 0, rng.integers(1, lim + 1, size=(nr, nc)))
    if variant == "big":
        assert dt == "i64"
        u = (1 << 61) - 256 + u          # C <= u + S < 2^61 - 128
        v = np.where(taken, -((1 << 61) - 64) - v, 0)
    elif variant == "ends":
        assert dt == "i32" and nr >= 4
        low = np.arange(nr) % 2 == 1     # odd rows near INT32_MIN, even rows near INT32_MAX
        u = np.where(low, I32.min + 128 + u, I32.max - 64 - u)
        il = nr // 2 + 1 if (nr // 2 + 1) % 2 else nr // 2   # an odd row: its chosen entry is INT32_MIN
        u[il], v[col[il]] = I32.min + 32, -32
    else:
        assert variant == "plain"
    C = u[:, None] + v[None, :] + S
    if variant == "ends":
        ih = 0 if col[0] != nc - 1 else 2                    # an even row: an entry not chosen is INT32_MAX
        C[ih, nc - 1] = I32.max
        assert C.min() == I32.min and C.max() == I32.max
    if variant == "plain":
        assert np.abs(C).max() <= 128 and u.min() >= 0 and u.max() <= 64 and v.min() >= -64 and v.max() <= 0
    stored = store(C, dt)
    assert np.array_equal(widen(stored, dt), C), "the cast must be exact"
    dual = np.float64 if dt in FLOATS else np.int64
    return Instance(dt, variant, *_frozen(stored, col, u.astype(dual), v.astype(dual)))


def depth(i, j):
    """The d of the plant at (i, j): 1 .. 32, different for neighbours."""
    return 1 + (3 * i + 5 * j) % 32


def plant_value(inst, i, j, d=None):
    """u[i] + v[j] - d as a widened value (int or float) that the dtype holds
    exactly.  multiscale: d in units of 1e300, below every rounding error of
    an instance whose entries reach 1e299 (errors of 1e283)."""
    d = depth(i, j) if d is None else d
    assert d >= 1
    if inst.variant == "multiscale":
        return float((inst.u[i] + inst.v[j]) - d * 1e300)
    x = int(inst.u[i]) + int(inst.v[j]) - d
    back = widen(store(np.array([x], dtype=np.float64 if inst.dt in FLOATS else np.int64), inst.dt), inst.dt)
    assert int(back[0]) == x and (inst.dt != "i32" or I32.min <= x <= I32.max), (inst.dt, x)
    return float(x) if inst.dt in FLOATS else x


def planted(inst, i, j, d=None):
    """The widened matrix (int64 / float64) with the plant at (i, j)."""
    W = widen(inst.S, inst.dt).copy()
    W[i, j] = plant_value(inst, i, j, d)
    return W


# --------------------------------------------------------------------------- the launch, mirrored
Geometry = collections.namedtuple("Geometry", "VEC NCAP QMAX chunks rows_per grid_y TX TY")
CERT_WG, SH_MAX_N, SH_MAX_N_LARGE = 256, 1024, 4096


def geometry(B, NR, NC, nc_live, itemsize, aligned=True):
    """launch_lsap_check's choices for a [B, NR, NC] batch of `itemsize`-byte
    costs and lsap_slack_kernel's thread shape for an instance of nc_live
    columns.  aligned: the cost pointer is a multiple of 16."""
    full = 16 // itemsize
    VEC = full if aligned and NC % full == 0 else 1
    NCAP = SH_MAX_N if NC <= SH_MAX_N else SH_MAX_N_LARGE
    QMAX = (NCAP + CERT_WG * VEC - 1) // (CERT_WG * VEC)
    chunks = min(max(1, 2048 // B), (NR + 7) // 8)
    rows_per = (NR + chunks - 1) // chunks
    grid_y = (NR + rows_per - 1) // rows_per
    groups = (nc_live + VEC - 1) // VEC
    lx = 0
    while (1 << lx) < groups and lx < 8:
        lx += 1
    return Geometry(VEC, NCAP, QMAX, chunks, rows_per, grid_y, 1 << lx, CERT_WG >> lx)


def position_rows(g, nr):
    rows = {0, g.TY - 1, g.TY, g.rows_per - 1, g.rows_per, 2 * g.rows_per - 1, (g.grid_y - 1) * g.rows_per, nr - 1}
    return sorted(i for i in rows if 0 <= i < nr)


def position_cols(g, nc):
    cols = {0, g.VEC - 1, g.VEC, g.TX * g.VEC - 1, g.TX * g.VEC, nc - g.VEC - 1, nc - g.VEC, nc - 1}
    for k in range(1, g.QMAX + 1):
        cols |= {k * CERT_WG * g.VEC - 1, k * CERT_WG * g.VEC}
    return sorted(j for j in cols if 0 <= j < nc)


def positions(g, nr, nc):
    """The entries (i, j) of an nr x nc corner at the edges of geometry g."""
    return [(i, j) for i in position_rows(g, nr) for j in position_cols(g, nc)]


def stripe(g, j):
    """The q of lsap_slack_kernel's register stripes that holds column j."""
    return (j // g.VEC) // g.TX


# --------------------------------------------------------------------------- the case list
# shapes: None, or the (nr_b, nc_b) of the members of a ragged batch.  large: through check_duals_large.
Case = collections.namedtuple("Case", "name dt variant B NR NC shapes large aligned")


def case_id(c):
    return f"{c.name}-{c.dt}-{c.B}x{c.NR}x{c.NC}" + ("" if c.variant == "plain" else "-" + c.variant)


RAGGED = ((20, 40), (13, 33), (0, 0), (1, 1), (7, 39), (20, 25))
RAGGED_LARGE = ((12, 2056), (9, 2049), (0, 0), (1, 1))


def _cases():
    out = []
    for dt in DTYPES:
        add = lambda name, B, NR, NC, variant="plain", shapes=None, large=False, aligned=True: out.append(  # noqa: E731
            Case(name, dt, variant, B, NR, NC, shapes, large, aligned))
        add("vec", 3, 20, 40)                      # VEC = 16 / itemsize; TY = rows_per or beyond
        add("odd", 3, 20, 39)                      # VEC = 1: NC % VEC != 0
        add("unaligned", 3, 20, 40, aligned=False)  # VEC = 1: the pointer
        add("few_cols", 3, 5, 8)                   # TX < 256, TY > rows_per
        add("last_stripe", 2, 24, 1024)            # NCAP = 1024, q = QMAX - 1 > 0 where VEC <= 2
        add("last_stripe_odd", 2, 24, 1023)        # ... and with VEC = 1, QMAX = 4
        add("short_chunk", 1, 300, 320)            # 38 chunks of 8 rows, the last holding 4
        add("mid_batch", 64, 300, 304)             # 2048 / B = 32 bounds the chunks: 30 of 10 rows
        add("wide", 2, 12, 4096, large=True)       # NCAP = 4096, q = QMAX - 1 for VEC 2 / 4 / 8
        add("wide_odd", 2, 12, 4095, large=True)   # ... and for VEC = 1, QMAX = 16
        add("wide_1032", 2, 12, 1032, large=True)  # the first NC % 8 == 0 above SH_MAX_N
        if ITEMSIZE[dt] == 2:
            add("wide_2056", 2, 12, 2056, large=True)  # VEC = 8: one pack in the last stripe
        add("ragged", len(RAGGED), 20, 40, shapes=RAGGED)
        add("ragged", len(RAGGED), 20, 40, shapes=RAGGED, large=True)
        add("ragged_large", len(RAGGED_LARGE), 12, 2056, shapes=RAGGED_LARGE, large=True)
    out.append(Case("vec", "i64", "big", 3, 20, 40, None, False, True))
    out.append(Case("vec", "i32", "ends", 3, 20, 36, None, False, True))
    out.append(Case("vec", "f64", "multiscale", 3, 20, 40, None, False, True))
    out.append(Case("odd", "f64", "multiscale", 3, 20, 39, None, False, True))
    return out


CASES = _cases()

# B >= 2048: one chunk per instance, every entry of the corner planted in exactly one instance
EXHAUSTIVE = ([(dt, 32, 64, True) for dt in DTYPES] +        # B = 2048, VEC 2 / 4 / 8
              [(dt, 44, 48, True) for dt in DTYPES] +        # B = 2112, not a power of two
              [(dt, 43, 49, True) for dt in ("i64", "f32", "bf16")] +   # VEC = 1, odd NC; B = 2107
              [(dt, 32, 64, False) for dt in ("i32", "f16")])           # VEC = 1, the pointer


def member_shape(case, b):
    return (case.NR, case.NC) if case.shapes is None else case.shapes[b]


def member(case, b):
    """The certified instance that is member b of the case's batch, None for an empty one."""
    nr, nc = member_shape(case, b)
    if nr == 0:
        return None
    return certified(case.dt, nr, nc, b % SEEDS if case.shapes is None else b, case.variant)


def case_geometry(case, b=0):
    return geometry(case.B, case.NR, case.NC, member_shape(case, b)[1], ITEMSIZE[case.dt], case.aligned)


def case_positions(case, b=0):
    nr, nc = member_shape(case, b)
    return positions(case_geometry(case, b), nr, nc) if nr else []


def poison(dt):
    """What the padding of a ragged batch holds, widened: a cost whose slack
    would be hugely negative, NaN for floats."""
    return np.nan if dt in FLOATS else (I32.min if dt == "i32" else -(1 << 60))


def batch(case):
    """-> (S [B, NR, NC] stored, col int64 [B, NR], u [B, NR], v [B, NC]), the
    padding of a ragged member poisoned: cost `poison`, duals NaN or 2^61 (a
    RANGE flag if read), col -1 as the entries require."""
    flt = case.dt in FLOATS
    dual = np.float64 if flt else np.int64
    pad = store(np.array(poison(case.dt), dtype=np.float64 if flt else np.int64), case.dt)[()]
    S = np.full((case.B, case.NR, case.NC), pad, dtype=STORE[case.dt])
    col = np.full((case.B, case.NR), -1, dtype=np.int64)
    u = np.full((case.B, case.NR), np.nan if flt else 1 << 61, dtype=dual)
    v = np.full((case.B, case.NC), np.nan if flt else 1 << 61, dtype=dual)
    for b in range(case.B):
        m = member(case, b)
        if m is not None:
            nr, nc = m.S.shape
            S[b, :nr, :nc], col[b, :nr], u[b, :nr], v[b, :nc] = m.S, m.col, m.u, m.v
    return S, col, u, v


# --------------------------------------------------------------------------- the input for the float gap
@functools.lru_cache(maxsize=None)
def gap_input(nr=300, nc=513):
    """(C float64 [nr, nc] of float32 values, col, u, v) with nothing feasible
    about it: three sums whose bits depend on the order of summation, over
    enough elements for the stride 256 and all four waves to take part."""
    rng = _rng(2, nr, nc, 0)
    scale = lambda n: 10.0 ** rng.integers(-3, 4, size=n)  # noqa: E731
    C = (rng.standard_normal((nr, nc)) * scale((nr, nc))).astype(np.float32).astype(np.float64)
    col = rng.permutation(nc)[:nr].astype(np.int64)
    u = rng.standard_normal(nr) * scale(nr)
    v = rng.standard_normal(nc) * scale(nc)
    # +-2^54 in waves 1 and 2 (the order of the waves decides whether wave 0's or wave 3's low bits survive), +-2^53 at
    # t and t + 256 (one thread adds both; an ascending sum carries 2^53 through everything between)
    chosen = C[np.arange(nr), col]
    for x in (u, v, chosen):
        x[70], x[140], x[7], x[263] = 2.0 ** 54, -2.0 ** 54, 2.0 ** 53, -2.0 ** 53
    C[np.arange(nr), col] = chosen
    assert np.array_equal(C.astype(np.float32).astype(np.float64), C)
    return _frozen(C, col, u, v)
