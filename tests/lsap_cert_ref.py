"""TEST INFRASTRUCTURE ONLY: the min-sum certificate (lsap_check_duals_,
lsap_check_duals_large_) on the host, written from the comment block above
SH_CERT_COL in include/santa_hip.h and from nothing else (no GPU, no library).

cert_ref(C, col, u, v, shape=None) -> (smin, tmax, gap, flags) of ONE wide
instance: C [NR, NC] int64, int32 or a float matrix already widened to float64,
col [NR], u [NR], v [NC] (int64 or float64), shape = (nr_b, nc_b) of a ragged
member.

Integers are Python integers in object arrays, so nothing wraps; where every
|u|, |v| and |C| is below 2^61 the slack matrix alone is taken in int64, whose
three terms then stay below 2^63 (python_integers=True takes it in object
arrays too; test_lsap_cert_cpu.py compares the two).  The library's
arithmetic does wrap; SH_CERT_RANGE marks every instance in which it could
have, and the other bits and the three values are then unspecified: callers
compare RANGE alone.  Floats are numpy float64, (C - u) - v in that order; the
minimum orders -0.0 below +0.0 and is NaN once a slack is; tmax keeps a NaN;
the gap's three sums are taken by `ordered_sum`, the header's order spelled
out.  A NaN is returned as numpy's default NaN: compare with `same_bits`,
which lets any NaN match any NaN.
"""
import numpy as np

COL, SLACK, TIGHT, SIGN, GAP, NONE, RANGE = 1, 2, 4, 8, 16, 32, 64
LIMIT = 1 << 61
WG, WAVE = 256, 64


def ordered_sum(x, idx, waves=(0, 1, 2, 3)):
    """The sum of the float64 elements x, element k belonging to slot idx[k]:
    thread t of 256 adds the elements of the slots t, t + 256, .. ascending;
    the 64 partial sums of a wave meet in the xor butterfly 32, 16, .. 1
    (x = x + x[lane ^ o]); the four waves' sums are added in the order `waves`
    (the header's is 0, 1, 2, 3; a test asks for another to show it matters)."""
    part = np.zeros(WG, dtype=np.float64)
    x, idx = np.asarray(x, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    turns = (int(idx.max()) // WG + 1) if idx.size else 0
    slot = np.zeros(turns * WG, dtype=np.float64)
    held = np.zeros(turns * WG, dtype=bool)
    slot[idx], held[idx] = x, True
    with np.errstate(all="ignore"):
        for k in range(turns):   # turn k: thread t adds slot t + 256 k if it holds an element
            part = np.where(held[k * WG:(k + 1) * WG], part + slot[k * WG:(k + 1) * WG], part)
        lane = np.arange(WG)
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[lane ^ o]   # (lane ^ o stays inside the wave: o < 64)
        total = part[WAVE * waves[0]]
        for w in waves[1:]:
            total = total + part[WAVE * w]
    return total


def float_min(x):
    """The minimum of a float64 array with -0.0 below +0.0; NaN if it holds one;
    +0.0 for an empty array."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size == 0:
        return np.float64(0.0)
    if np.isnan(x).any():
        return np.float64(np.nan)
    m = x.min()
    if m == 0 and np.signbit(x[x == 0]).any():
        return np.float64(-0.0)
    return np.float64(m)


def same_bits(a, b):
    """float64 values equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def cert_ref(C, col, u, v, shape=None, python_integers=False):
    C = np.asarray(C)
    NR, NC = C.shape
    integer = np.issubdtype(C.dtype, np.integer)
    zero = 0 if integer else np.float64(0.0)
    nr, nc = (NR, NC) if shape is None else (int(shape[0]), int(shape[1]))
    col = [int(c) for c in np.asarray(col)]
    if not (1 <= nr <= nc and nc <= NC and nr <= NR):
        if not (nr == 0 and 0 <= nc <= NC):
            return zero, zero, zero, COL          # a shape outside the padded matrix
    flags = 0
    if any(c != -1 for c in col[nr:]):
        flags |= COL                              # a padded row whose col is not -1
    live = col[:nr]
    if nr >= 1 and all(c == -1 for c in live):
        return zero, zero, zero, NONE             # nothing else is checked
    if any(c == -1 for c in live):
        flags |= COL                              # a live row without a column next to one with
    valid = [i for i, c in enumerate(live) if 0 <= c < nc]
    if any(c != -1 and not 0 <= c < nc for c in live):
        flags |= COL
    taken = [live[i] for i in valid]
    if len(set(taken)) != len(taken):
        flags |= COL                              # a column taken twice
    if integer:
        out = _integers(C, u, v, nr, nc, valid, taken, python_integers)
    else:
        out = _floats(C, u, v, nr, nc, valid, taken)
    return out[0], out[1], out[2], flags | out[3]


def _integers(C, u, v, nr, nc, valid, taken, python_integers=False):
    wide_costs = C.dtype.itemsize == 8
    Cl = C[:nr, :nc]
    ul, vl = np.asarray(u)[:nr].astype(object), np.asarray(v)[:nc].astype(object)
    flags = 0
    if any(abs(x) >= LIMIT for x in ul) or any(abs(x) >= LIMIT for x in vl):
        flags |= RANGE
    big_cost = bool(Cl.size) and max(abs(int(Cl.max())), abs(int(Cl.min()))) >= LIMIT
    if wide_costs and big_cost:
        flags |= RANGE
    if not Cl.size:
        smin = 0
    elif flags & RANGE or big_cost or python_integers:
        smin = int(((Cl.astype(object) - ul[:, None]) - vl[None, :]).min())
    else:   # three terms below 2^61 each: below 2^63, int64 cannot wrap either
        smin = int(((Cl.astype(np.int64) - np.asarray(u, dtype=np.int64)[:nr, None])
                    - np.asarray(v, dtype=np.int64)[None, :nc]).min())
    chosen = [int(Cl[i, j]) for i, j in zip(valid, taken)]
    tmax = max([abs((c - ul[i]) - vl[j]) for c, i, j in zip(chosen, valid, taken)], default=0)
    gap = (sum(ul) + sum(vl)) - sum(chosen)
    free = np.ones(nc, dtype=bool)
    free[taken] = False
    if any(x > 0 for x in vl) or any(x != 0 for x in vl[free]):
        flags |= SIGN
    if smin < 0:
        flags |= SLACK
    if tmax != 0:
        flags |= TIGHT
    if gap != 0:
        flags |= GAP
    return int(smin), int(tmax), int(gap), flags


def _floats(C, u, v, nr, nc, valid, taken):
    Cl = np.asarray(C, dtype=np.float64)[:nr, :nc]
    ul, vl = np.asarray(u, dtype=np.float64)[:nr], np.asarray(v, dtype=np.float64)[:nc]
    valid, taken = np.asarray(valid, dtype=np.int64), np.asarray(taken, dtype=np.int64)
    flags = 0
    with np.errstate(all="ignore"):
        smin = float_min((Cl - ul[:, None]) - vl[None, :])
        chosen = Cl[valid, taken]
        tight = np.abs((chosen - ul[valid]) - vl[taken])
        tmax = np.float64(0.0)
        if tight.size:
            tmax = np.float64(np.nan) if np.isnan(tight).any() else np.float64(tight.max())
        su = ordered_sum(ul, np.arange(nr))
        sv = ordered_sum(vl, np.arange(nc))
        sc = ordered_sum(chosen, valid)
        gap = np.float64((su + sv) - sc)
    free = np.ones(nc, dtype=bool)
    free[taken] = False
    if (vl > 0).any() or (vl[free] != 0).any():
        flags |= SIGN
    if not smin >= 0:
        flags |= SLACK
    if not tmax == 0:
        flags |= TIGHT
    return smin, tmax, gap, flags
