"""The host reference of the min-sum certificate (lsap_cert_ref.cert_ref) and
the instances of lsap_cert_families.py, proved without the library: the
reference on honest solves (the replay's duals), on instances certified by
construction and under every plant, the float gap's summation order, and that
the case list of test_lsap_cert_gpu.py reaches every class of launch."""
import math
import os
import re

import numpy as np
import pytest

import lsap_cert_families as CF
import lsap_duals_ref as R
import lsap_families as F
from lsap_cert_ref import (COL, GAP, NONE, RANGE, SIGN, SLACK, TIGHT, cert_ref, float_min, ordered_sum,
                           same_bits)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "santa_hip.h")


def test_flag_values_are_the_headers():
    text = open(HEADER).read()
    got = {name: int(val) for name, val in re.findall(r"#define SH_CERT_(\w+) (\d+)", text)}
    assert got == {"COL": COL, "SLACK": SLACK, "TIGHT": TIGHT, "SIGN": SIGN, "GAP": GAP, "NONE": NONE, "RANGE": RANGE}


# --------------------------------------------------------------------------- honest solves
HONEST = [(f, "int64", nr, nc) for f in ("mw", "mw_neg", "two_scale43", "neg_cols", "window_edges", "i32_extremes")
          for nr, nc in ((20, 20), (17, 33))]
HONEST += [(f, "int32", 17, 33) for f in ("mw", "i32_extremes")]
HONEST += [(f, "float64", nr, nc) for f in ("mw_tenths", "decimal", "multiscale", "subnormal64")
           for nr, nc in ((20, 20), (17, 33))]


@pytest.mark.parametrize("family,dtype,nr,nc", HONEST, ids=lambda x: str(x))
def test_reference_on_the_replays_duals(family, dtype, nr, nc):
    C = F.instance(family, "int64" if dtype == "int32" else dtype, nr, nc, 1)
    if dtype == "int32":
        C = C.astype(np.int32)
        assert np.array_equal(C.astype(np.int64), F.instance(family, "int64", nr, nc, 1))
    col, u, v = R.replay(C)
    smin, tmax, gap, flags = cert_ref(C, col, u, v)
    if dtype != "float64":
        assert all(R.invariants(C, col, u, v).values())
        assert (smin, tmax, gap, flags) == (0, 0, 0, 0)
        assert smin == int((C.astype(object) - u.astype(object)[:, None] - v.astype(object)[None, :]).min())
        return
    slack = (C - u[:, None]) - v[None, :]
    assert same_bits(smin, slack.min()) or (smin == 0 and slack.min() == 0)   # (numpy's min does not order the zeros)
    assert same_bits(tmax, np.abs(slack[np.arange(nr), col]).max())
    assert not flags & (COL | SIGN | NONE | RANGE | GAP)
    assert bool(flags & SLACK) == bool(slack.min() < 0) and bool(flags & TIGHT) == bool(tmax != 0)
    assert abs(gap) <= 1e-9 * max(1.0, np.abs(u).sum() + np.abs(v).sum())


# --------------------------------------------------------------------------- certified instances and plants
def _members():
    seen = {}
    for c in CF.CASES:
        for b in range(c.B):
            m = CF.member(c, b)
            if m is not None and c.variant != "multiscale":
                seen.setdefault((c.dt, c.variant) + m.S.shape + (b % CF.SEEDS if c.shapes is None else b,), (c, b))
    return list(seen.values())


def test_certified_instances_certify_and_every_plant_is_seen():
    """flags 0 and (0, 0, 0) on every member of every case; under each plant of
    the case's positions the minimum is -d and the flags are SLACK alone, or
    SLACK | TIGHT | GAP where the position is a chosen entry (floats: SLACK |
    TIGHT, and the gap d all the same)."""
    n_plants = n_chosen = 0
    for c, b in _members():
        m = CF.member(c, b)
        W = CF.widen(m.S, m.dt)
        assert cert_ref(W, m.col, m.u, m.v) == (0, 0, 0, 0), CF.case_id(c)
        for i, j in CF.case_positions(c, b):
            d = CF.depth(i, j)
            P = CF.planted(m, i, j)
            assert (P != W).sum() == 1 and P[i, j] == m.u[i] + m.v[j] - d
            P = P.astype(np.int32) if m.dt == "i32" else P
            smin, tmax, gap, flags = cert_ref(P, m.col, m.u, m.v)
            if m.dt in ("i64", "i32") and m.S.size <= 1024:   # the slack matrix in Python integers: the same
                assert cert_ref(P, m.col, m.u, m.v, python_integers=True) == (smin, tmax, gap, flags)
            chosen = m.col[i] == j
            both = SLACK | TIGHT | (0 if m.dt in CF.FLOATS else GAP)   # (GAP is a bit of the integer entries)
            assert smin == -d and flags == (both if chosen else SLACK), (CF.case_id(c), b, i, j)
            assert (tmax, gap) == ((d, d) if chosen else (0, 0))
            n_plants += 1
            n_chosen += chosen
    assert n_plants > 2000 and n_chosen >= 1


def test_a_plant_on_a_chosen_entry():
    for dt in CF.DTYPES:
        m = CF.certified(dt, 9, 12, 0)
        i, j = 4, int(m.col[4])
        want = SLACK | TIGHT | (0 if dt in CF.FLOATS else GAP)
        assert cert_ref(CF.planted(m, i, j, 7), m.col, m.u, m.v) == (-7, 7, 7, want)


def test_multiscale_instances_are_feasible_only_up_to_rounding():
    m = CF.certified("f64", 20, 40, 0, "multiscale")
    smin, tmax, gap, flags = cert_ref(m.S, m.col, m.u, m.v)
    slack = (m.S - m.u[:, None]) - m.v[None, :]
    assert same_bits(smin, slack.min()) and smin < 0 and flags & SLACK   # rounding shows: the reference decides
    i, j = next((i, j) for i, j in CF.positions(CF.geometry(3, 20, 40, 40, 8), 20, 40) if m.col[i] != j)
    P = CF.planted(m, i, j)
    got = cert_ref(P, m.col, m.u, m.v)
    assert same_bits(got[0], (P[i, j] - m.u[i]) - m.v[j]) and got[0] < smin and got[3] & SLACK


def test_reference_flags():
    m = CF.certified("i64", 6, 9, 0)
    W, col, u, v = CF.widen(m.S, "i64"), m.col.copy(), m.u.copy(), m.v.copy()
    free = int(np.setdiff1d(np.arange(9), col)[0])

    def ref(**kw):
        return cert_ref(kw.get("W", W), kw.get("col", col), kw.get("u", u), kw.get("v", v), kw.get("shape"))

    def changed(a, k, x):
        a = a.copy()
        a[k] = x
        return a
    assert ref(col=np.full(6, -1)) == (0, 0, 0, NONE)
    assert ref(col=changed(col, 2, -1))[3] & COL and ref(col=changed(col, 2, 9))[3] & COL
    assert ref(col=changed(col, 2, -2))[3] & COL and ref(col=changed(col, 2, col[3]))[3] & COL
    assert ref(col=changed(col, 2, free))[3] & (COL | TIGHT) == TIGHT
    assert ref(v=changed(v, free, -1))[3] == SIGN | GAP and ref(v=changed(v, free, -1))[2] == -1
    assert ref(v=changed(v, int(col[0]), 1))[3] & SIGN
    assert ref(u=changed(u, 1, u[1] - 3)) == (0, 3, -3, TIGHT | GAP)
    assert ref(u=changed(u, 1, u[1] + 3))[:3] == (-3, 3, 3)
    assert ref(u=changed(u, 1, 1 << 61))[3] & RANGE and ref(v=changed(v, 0, -(1 << 61)))[3] & RANGE
    assert ref(W=changed(W, (0, free), 1 << 61))[3] == RANGE
    assert not cert_ref(changed(W, (0, free), (1 << 31) - 1).astype(np.int32), col, u, v)[3]
    # shapes: the empty one, one outside the padded matrix, a corner whose outside is never read
    assert ref(shape=(0, 0), col=np.full(6, -1)) == (0, 0, 0, 0) and ref(shape=(0, 0)) == (0, 0, 0, COL)
    assert ref(shape=(0, 4), col=np.full(6, -1), v=np.zeros(9, dtype=np.int64)) == (0, 0, 0, 0)
    for shape in ((7, 9), (6, 10), (5, 4), (-1, 3), (0, 10)):
        assert ref(shape=shape) == (0, 0, 0, COL)
    n = CF.certified("i64", 4, 5, 1)
    W2, col2 = W.copy(), np.full(6, -1)
    W2[:4, :5], col2[:4] = CF.widen(n.S, "i64"), n.col
    W2[4:], W2[:, 5:] = -(1 << 62), -(1 << 62)
    u2, v2 = np.full(6, 1 << 61), np.full(9, 1 << 61)
    u2[:4], v2[:5] = n.u, n.v
    assert cert_ref(W2, col2, u2, v2, (4, 5)) == (0, 0, 0, 0)
    assert cert_ref(W2, changed(col2, 5, 0), u2, v2, (4, 5))[3] == COL


def test_reference_float_rules():
    assert same_bits(float_min([0.0, -0.0, 1.0]), -0.0) and same_bits(float_min([0.0, 1.0]), 0.0)
    assert np.isnan(float_min([1.0, np.nan, -np.inf])) and float_min([1.0, -np.inf]) == -np.inf
    assert same_bits(float_min([]), 0.0)
    m = CF.certified("f64", 6, 9, 0)
    W = m.S.copy()
    free = int(np.setdiff1d(np.arange(9), m.col)[0])
    W[2, free] = np.nan
    smin, tmax, gap, flags = cert_ref(W, m.col, m.u, m.v)
    assert np.isnan(smin) and flags == SLACK and same_bits(tmax, 0.0) and same_bits(gap, 0.0)
    W[2, m.col[2]] = np.nan
    smin, tmax, gap, flags = cert_ref(W, m.col, m.u, m.v)
    assert np.isnan(tmax) and np.isnan(gap) and flags == SLACK | TIGHT   # (floats have no GAP bit)
    W = m.S.copy()
    W[2, free] = np.inf
    assert cert_ref(W, m.col, m.u, m.v)[3] == 0
    W[3, free] = -np.inf
    assert cert_ref(W, m.col, m.u, m.v)[0] == -np.inf


# --------------------------------------------------------------------------- the float gap's order
def test_the_gaps_order_matters_on_the_gap_input():
    C, col, u, v = CF.gap_input()
    nr, nc = C.shape
    assert nr >= 300 and nc >= 513
    chosen = C[np.arange(nr), col]
    gap = cert_ref(C, col, u, v)[2]
    sums = [ordered_sum(u, np.arange(nr)), ordered_sum(v, np.arange(nc)), ordered_sum(chosen, np.arange(nr))]
    assert same_bits(gap, (sums[0] + sums[1]) - sums[2])

    def ascending(x):
        s = 0.0
        for y in x:
            s += float(y)
        return s
    assert not same_bits(gap, (ascending(u) + ascending(v)) - ascending(chosen))
    assert not same_bits(gap, (math.fsum(u) + math.fsum(v)) - math.fsum(chosen))
    for x, s in zip((u, v, chosen), sums):
        assert abs(s - math.fsum(x)) <= 1e-12 * np.abs(x).sum()    # a sum all the same
        assert not same_bits(s, ascending(x))
    # the order of the four waves alone decides bits too
    back = [ordered_sum(x, np.arange(len(x)), waves=(3, 2, 1, 0)) for x in (u, v, chosen)]
    assert not same_bits(gap, (back[0] + back[1]) - back[2])
    assert not any(same_bits(s, b) for s, b in zip(sums, back))


def test_ordered_sum_by_hand():
    x = np.arange(1.0, 601.0)
    assert ordered_sum(x, np.arange(600)) == x.sum()
    # thread 0 adds elements 0, 256, 512 in that order: 1 + 2^53 + (-2^53) = 0, not 1
    y = np.zeros(600)
    y[0], y[256], y[512] = 1.0, 2.0 ** 53, -2.0 ** 53
    assert ordered_sum(y, np.arange(600)) == 0.0
    y[0], y[256], y[512] = 2.0 ** 53, -2.0 ** 53, 1.0
    assert ordered_sum(y, np.arange(600)) == 1.0
    # the butterfly pairs lane 0 with lane 32 first, and wave 0 is added before wave 3
    z = np.zeros(256)
    z[0], z[32], z[1] = 2.0 ** 53, -2.0 ** 53, 1.0
    assert ordered_sum(z, np.arange(256)) == 1.0
    z[0], z[32], z[1], z[33] = 2.0 ** 53, 1.0, -2.0 ** 53, 0.0
    assert ordered_sum(z, np.arange(256)) == 0.0
    w = np.zeros(256)
    w[0], w[64], w[192] = 2.0 ** 53, 1.0, -2.0 ** 53
    assert ordered_sum(w, np.arange(256)) == 0.0 and ordered_sum(w, np.arange(256), waves=(0, 3, 1, 2)) == 1.0


# --------------------------------------------------------------------------- the geometry and the case list
def test_geometry_reproduces_the_launch_worked_out_by_hand():
    """(B, NR, NC, nc_live, itemsize, aligned) -> VEC, NCAP, QMAX, chunks,
    rows_per, grid_y, TX, TY, from launch_lsap_check (chunks = min(max(1,
    2048 / B), (NR + 7) / 8), rows_per and grid_y by rounding up) and
    lsap_slack_kernel (TX the power of two that covers ceil(nc / VEC), at
    most 256; TY = 256 / TX)."""
    table = {
        (3, 5, 8, 8, 8, True): (2, 1024, 2, 1, 5, 1, 4, 64),
        (3, 5, 8, 8, 2, True): (8, 1024, 1, 1, 5, 1, 1, 256),
        (1, 300, 320, 320, 8, True): (2, 1024, 2, 38, 8, 38, 256, 1),
        (64, 300, 304, 304, 4, True): (4, 1024, 1, 32, 10, 30, 128, 2),
        (2, 24, 1024, 1024, 8, True): (2, 1024, 2, 3, 8, 3, 256, 1),
        (2, 24, 1023, 1023, 8, True): (1, 1024, 4, 3, 8, 3, 256, 1),
        (2, 12, 4096, 4096, 2, True): (8, 4096, 2, 2, 6, 2, 256, 1),
        (2, 12, 4095, 4095, 4, True): (1, 4096, 16, 2, 6, 2, 256, 1),
        (2, 12, 1032, 1032, 4, True): (4, 4096, 4, 2, 6, 2, 256, 1),
        (2048, 32, 64, 64, 4, True): (4, 1024, 1, 1, 32, 1, 16, 16),
        (2112, 44, 48, 48, 2, True): (8, 1024, 1, 1, 44, 1, 8, 32),
        (2048, 32, 64, 64, 4, False): (1, 1024, 4, 1, 32, 1, 64, 4),
        (6, 20, 40, 33, 2, True): (8, 1024, 1, 3, 7, 3, 8, 32),
        (1000, 300, 300, 300, 8, True): (2, 1024, 2, 2, 150, 2, 256, 1),
    }
    for args, want in table.items():
        assert tuple(CF.geometry(*args)) == want, args


def test_positions_lie_on_the_edges():
    g = CF.geometry(2, 12, 4095, 4095, 8)
    P = CF.positions(g, 12, 4095)
    assert set(i for i, _ in P) == {0, 1, 5, 6, 11}
    cols = set(j for _, j in P)
    assert {0, 1, 255, 256, 511, 512, 3839, 3840, 4093, 4094} <= cols and max(cols) == 4094
    assert max(CF.stripe(g, j) for j in cols) == g.QMAX - 1 == 15
    assert all(0 <= i < 5 and 0 <= j < 8 for i, j in CF.positions(CF.geometry(3, 5, 8, 8, 8), 5, 8))


def test_the_case_list_reaches_every_class():
    ids = [CF.case_id(c) + ("-large" if c.large else "") for c in CF.CASES]
    assert len(set(ids)) == len(ids)
    G = [(c, b, CF.case_geometry(c, b), CF.case_positions(c, b)) for c in CF.CASES for b in range(c.B)
         if CF.member_shape(c, b)[0]]
    X = [(dt, CF.geometry(nr * nc, nr, nc, nc, CF.ITEMSIZE[dt], al)) for dt, nr, nc, al in CF.EXHAUSTIVE]

    def some(pred, dts=CF.DTYPES):
        return all(any(c.dt == dt and pred(c, g, P) for c, b, g, P in G) for dt in dts)
    top = lambda g, P: max(CF.stripe(g, j) for _, j in P)  # noqa: E731
    for dt in CF.DTYPES:   # VEC 2 / 4 / 8 by item size
        assert any(c.dt == dt and g.VEC == 16 // CF.ITEMSIZE[dt] for c, b, g, P in G)
        assert any(d == dt and g.VEC == 16 // CF.ITEMSIZE[dt] for d, g in X)
    assert some(lambda c, g, P: g.VEC == 1 and c.NC % 2 == 1)
    assert some(lambda c, g, P: g.VEC == 1 and not c.aligned and c.NC % (16 // CF.ITEMSIZE[c.dt]) == 0)
    assert any(g.VEC == 1 and nc % 2 for (dt, nr, nc, al), (_, g) in zip(CF.EXHAUSTIVE, X))
    assert any(g.VEC == 1 and not al for (dt, nr, nc, al), (_, g) in zip(CF.EXHAUSTIVE, X))
    assert some(lambda c, g, P: g.NCAP == 1024 and g.QMAX > 1 and top(g, P) == g.QMAX - 1)
    for vec in (1, 2, 4, 8):
        assert any(g.NCAP == 4096 and g.VEC == vec and top(g, P) == g.QMAX - 1 for c, b, g, P in G), vec
    assert some(lambda c, g, P: g.NCAP == 4096 and g.VEC == 1 and top(g, P) == 15)
    assert some(lambda c, g, P: g.NCAP == 4096 and g.VEC == 8 and c.NC == 2056 and top(g, P) == 1, ("f16", "bf16"))
    assert some(lambda c, g, P: g.TX < 256 and g.TY > g.rows_per)
    assert some(lambda c, g, P: g.TX < 256 and g.TY < g.rows_per)
    assert all(g.TX < 256 and g.TY < g.rows_per for _, g in X if g.VEC < 8) and any(
        g.VEC == 8 and g.TY < g.rows_per for _, g in X)
    assert some(lambda c, g, P: c.B == 1 and g.chunks == (c.NR + 7) // 8 and c.NR % g.rows_per == 4)
    assert some(lambda c, g, P: c.B == 64 and g.chunks == 2048 // c.B < (c.NR + 7) // 8 and g.grid_y > 1)
    assert all(g.chunks == 1 and g.grid_y == 1 and g.rows_per >= 2 * g.TY or g.VEC == 8 for _, g in X)
    Bs = [nr * nc for _, nr, nc, _ in CF.EXHAUSTIVE]
    assert min(Bs) >= 2048 and any(B & (B - 1) == 0 for B in Bs) and any(B & (B - 1) for B in Bs)
    for dt in CF.DTYPES:   # the ragged batch: a partial pack, an empty member, a 1 x 1 member
        for large in (False, True):
            r = [c for c in CF.CASES if c.dt == dt and c.shapes and c.large == large and c.NC == 40]
            assert len(r) == 1 and CF.geometry(r[0].B, 20, 40, 33, CF.ITEMSIZE[dt]).VEC > 1
            assert (0, 0) in r[0].shapes and (1, 1) in r[0].shapes
            assert any(nr < 20 and nc < 40 and nc % 2 for nr, nc in r[0].shapes)
    # every row of a chunk's edge and every stripe's edge is a position somewhere; no tensor is large
    assert all(c.B * c.NR * c.NC * CF.ITEMSIZE[c.dt] <= 48 << 20 for c in CF.CASES)
    assert all((nr * nc) ** 2 * CF.ITEMSIZE[dt] <= 40 << 20 for dt, nr, nc, _ in CF.EXHAUSTIVE)


def test_batches_pad_with_poison():
    c = next(c for c in CF.CASES if c.shapes and c.dt == "bf16" and not c.large)
    S, col, u, v = CF.batch(c)
    W = CF.widen(S, "bf16")
    for b, (nr, nc) in enumerate(c.shapes):
        assert np.isnan(W[b, nr:]).all() and np.isnan(W[b, :, nc:]).all() and not np.isnan(W[b, :nr, :nc]).any()
        assert (col[b, nr:] == -1).all() and np.isnan(u[b, nr:]).all() and np.isnan(v[b, nc:]).all()
        want = (0, 0, 0, 0)
        assert cert_ref(W[b], col[b], u[b], v[b], (nr, nc)) == want
    c = next(c for c in CF.CASES if c.shapes and c.dt == "i32" and not c.large)
    S, col, u, v = CF.batch(c)
    assert (S[1, 13:] == CF.I32.min).all() and cert_ref(S[1], col[1], u[1], v[1], (13, 33)) == (0, 0, 0, 0)
    assert cert_ref(S[1], col[1], u[1], v[1], (14, 33))[3] & RANGE    # one row further the poison is read
