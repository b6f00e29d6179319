"""santa_sp3_kernel's step after its instruction diet: the
priority thresholds behind one test at the loop head, the key field's bias
carried in state (u_l = u + BIAS, Wp = (W << 11) + 2^31), an entry's value by
one 24-bit multiply, and the winner's lane mask taken from the compare -- on
crafted blocks, in the pattern of test_sp3_dijkstra_loop_gpu.py.

Every case first asserts on the CPU (sap_duals below, scipy's solve as
lsap_families.sap_trace runs it, checked against it) the property that makes
it meaningful; then the sparse kernel (SH_FLAG_SP_TILE) must equal the
oracle's round: col, exact cost, per-block steps, the new type vector and the
happiness deltas.

Two premises of the kind asked for cannot occur in this solve and are
asserted in the form that can: a column dual only ever falls (W = -v only
rises: the update is minVal - spc >= 0), so "W moves in both directions" is
W moved and W unmoved; and a row reached as a non-first step is an assigned
row, whose own Dijkstra ran before (rows start in index order), so what the
peeled step's "u~ = 0" rests on is that no row's dual is touched before its
own Dijkstra, while rows are reached as non-first steps afterwards."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lsap_families import sap_trace  # noqa: E402
from test_sp3_dijkstra_loop_gpu import chain, runs_block  # noqa: E402
from test_sp3_first_step_gpu import (FILL0, NG, NW, OVF_CAP, check_blocks, cost_v, crafted,  # noqa: E402,F401
                                     dijkstra_lengths, sh, small, small_ctx)

pytestmark = pytest.mark.gpu

PRIO = (32, 8, 2)  # SP3_PRIO_A, B, C: the priority falls at Dijkstra n - 32, n - 8, n - 2


# -- scipy's solve with its duals -----------------------------------------------------------

def sap_duals(C):
    """scipy's solve (sap_trace's decisions).  Returns a dict: `steps` per
    Dijkstra [(row, winner's position in `remaining`, len(remaining), winner)],
    `u`, `v` the final duals, `u0` each row's dual when its own Dijkstra starts,
    `ut` the u~ = u[i] - minVal every non-first step reads, `W` the column
    duals -v after every Dijkstra."""
    C = np.ascontiguousarray(C, dtype=np.int64)
    nr, nc = C.shape
    INF = np.iinfo(np.int64).max
    u, v = np.zeros(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64)
    path = -np.ones(nc, dtype=np.int64)
    col4row, row4col = -np.ones(nr, dtype=np.int64), -np.ones(nc, dtype=np.int64)
    steps, u0, ut, Ws = [], [], [], []
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1)
        spc = np.full(nc, INF, dtype=np.int64)
        SR, SC, rec = [], [], []
        minVal, i = 0, cur
        u0.append(int(u[cur]))
        while True:
            if SR:
                ut.append(int(u[i]) - minVal)
            SR.append(i)
            r = minVal + C[i, remaining] - u[i] - v[remaining]
            upd = r < spc[remaining]
            s = np.where(upd, r, spc[remaining])
            spc[remaining] = s
            path[remaining[upd]] = i
            minVal = int(s.min())
            at = np.flatnonzero(s == minVal)
            free = at[row4col[remaining[at]] < 0]
            index = int(free[-1] if free.size else at[0])
            j = int(remaining[index])
            rec.append((i, index, len(remaining), j))
            SC.append(j)
            remaining[index] = remaining[-1]
            remaining = remaining[:-1]
            if row4col[j] < 0:
                break
            i = int(row4col[j])
        u[cur] += minVal
        others = np.array(SR[1:], dtype=np.int64)
        u[others] += minVal - spc[col4row[others]]
        SCa = np.array(SC, dtype=np.int64)
        v[SCa] -= minVal - spc[SCa]
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
        steps.append(rec)
        Ws.append(-v.copy())
    assert np.array_equal(col4row, sap_trace(C)[0])
    return dict(steps=steps, u=u, v=v, u0=u0, ut=np.array(ut, dtype=np.int64), W=np.array(Ws))


def lattice(M=199):
    """LatticeRange's constants (M = 199 at n_wish = 100)."""
    m3 = max(1, (M - 1) // 3)
    cw = m3.bit_length() - 1
    bu = max(1, M - 1 - (1 << cw)).bit_length() - 1
    assert (1 << cw) + 1 + (1 << bu) <= M
    return ((1 << 19) + (1 << bu) - 1, 0xFFF00000 | (511 & ~((2 << bu) - 1)),
            (1 << 18) + (1 << cw) - 1, 0xFFF80000 | (511 & ~((2 << cw) - 1)))


def leaves_range(T):
    """Whether the kernel's checks send the block to the fallback launch: the
    u~ of every non-first step, every column dual after every Dijkstra and the
    final row duals, as LatticeRange's bit tests."""
    CU, MU, CW, MW = lattice()
    bad_u = ((np.concatenate([T["ut"], T["u"]]) + CU) & 0xFFFFFFFF & MU) != 0
    bad_w = ((T["W"].reshape(-1) + CW) & 0xFFFFFFFF & MW) != 0
    return bool(bad_u.any() or bad_w.any())


def at_ranks(ranks):
    """A full wishlist holding gift type t at rank a (position NW - a) for
    every (t, a) of `ranks`, filler types that no block holds elsewhere."""
    h = [None] * NW
    for t, a in ranks:
        assert 1 <= a <= NW and h[NW - a] is None
        h[NW - a] = int(t)
    fill = iter(range(FILL0, NG - 1))
    return [x if x is not None else next(fill) for x in h]


def run(sh, sd, wish, types, rows, extra=0):
    from santa_hip import _lib
    c = small_ctx(sh, sd, wish)
    steps = check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE | extra)
    c.close()
    return steps


# -- the loop head's priority thresholds ---------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 8, 9, 31, 32, 33, 34, 256])
def test_loop_head(sh, small, n):
    """The thresholds n - 32, n - 8, n - 2 lie below 0, at 0, on the first and
    on the last Dijkstras over these n.  Every threshold index, the index
    before it and the block's last index hold a multi-step Dijkstra where one
    can stand (the first Dijkstra of a block is always single-step); the rest
    are single-step, so the inner loop is entered and left around every
    threshold."""
    sd, _ = small
    th = [n - p for p in PRIO]
    multi = sorted({j for t in th for j in (t - 1, t) if 1 <= j < n} | {n - 1})
    assert (n - PRIO[0] < 0) == (n < 32) and (n - PRIO[0] == 0) == (n == 32)
    assert n < 8 or any(t in multi and t - 1 in multi for t in th)
    kinds = [2 if j in multi else 1 for j in range(n)]
    wish, types, rows = runs_block(sd, n, kinds)
    S, _ = dijkstra_lengths(cost_v(wish[rows[0]], types[rows[0]]))
    assert len(S) == n and ((S == 1) == (np.asarray(kinds) == 1)).all()
    run(sh, sd, wish, types, rows)


# -- the bias carried in state ---------------------------------------------------------------

def duals_block(sd, n=67):
    """Rows A = 0 (column 0 at rank 2, column 1 at rank 1), B = 1 (column 0 at
    rank 100, column 2 at rank 99) and D = 2 (column 0 at rank 1): B pushes A
    off column 0 or takes column 2 at the same value, the dual of column 0
    falls by one rank, and D's path over column 0 ends on a tight edge: its
    dual ends 0.  Rows 3 .. 9 miss every column (dual 1), the rest want a
    column of their own at ranks 1 .. 100 (dual < 0)."""
    heads = [at_ranks([(0, 2), (1, 1)]), at_ranks([(0, 100), (2, 99)]), at_ranks([(0, 1)])]
    heads += [at_ranks([]) for _ in range(3, 10)]
    heads += [at_ranks([(j, 1 + (7 * j) % NW)]) for j in range(10, n)]
    return crafted(sd, np.arange(n), heads)


def ladder_block(sd, k, n=40):
    """k levels of two rows that both want column j at rank 100 and column
    j + 1 at rank 1: the loser of a level falls to the next one or to a miss,
    and the contested columns' duals fall by a whole wishlist (100 ranks),
    the largest a dual gets in a square block (see test_bias)."""
    heads = []
    for j in range(k):
        heads += [at_ranks([(j, NW), (j + 1, 1)])] * 2
    heads += [at_ranks([(k + 1 + t, NW)]) for t in range(n - 2 * k)]
    return crafted(sd, np.arange(n), heads)


def bias_blocks(sd):
    return {"duals": duals_block(sd), "ladder5": ladder_block(sd, 5), "ladder6": ladder_block(sd, 6)}


@pytest.mark.parametrize("test_range", [False, True])
@pytest.mark.parametrize("name", ["duals", "ladder5", "ladder6"])
def test_bias(sh, small, name, test_range):
    """Row duals that end negative, zero and positive, column duals that move
    and that stay; no row's dual is touched before its own Dijkstra (the
    peeled step's u~ = 0) while rows are read as non-first steps afterwards;
    the largest duals a block reaches -- each also under SH_FLAG_TEST_RANGE,
    where the fallback launch solves the block.  The exact cost is read from
    u_l + v: a lost constant shows there.

    A block that leaves the lattice range by itself was asked for and cannot
    be crafted from wishlists: until the last Dijkstra ends an unassigned
    column with v = 0 remains, so every row dual is at most a miss (1) and
    every column dual at least -(100 * 512 + 1) -- |A| <= 100 against the
    checked 512 and 1024, which the ladder blocks reach and assert; the
    range's far side is run by SH_FLAG_TEST_RANGE alone, as before."""
    from santa_hip import _lib
    sd, _ = small
    wish, types, rows = bias_blocks(sd)[name]
    C = cost_v(wish[rows[0]], types[rows[0]])
    T = sap_duals(C)
    assert all(x == 0 for x in T["u0"]) and len(T["ut"]) > 0
    if name == "duals":
        assert T["u"][2] == 0 and (T["u"][3:10] == 1).all() and (T["u"][10:] < 0).all()
        assert T["v"][0] < 0 and (T["W"][-1] > 0).any() and (T["W"][-1] == 0).any()
        assert (np.diff(T["W"], axis=0) >= 0).all()  # (a column dual only falls)
        assert (T["ut"] != 0).any() and not leaves_range(T)
        hit = C[1][C[1] < 0]
        assert sorted(hit.tolist()) == [-NW * 512, -(NW - 1) * 512]
    else:
        top = int(np.abs(T["W"]).max()) >> 9  # (ranks: the A part of the largest column dual)
        assert top == NW and (np.abs(T["ut"]).max() >> 9) >= NW - 1 and not leaves_range(T)
    run(sh, sd, wish, types, rows, _lib.SH_FLAG_TEST_RANGE if test_range else 0)


# -- an entry's value --------------------------------------------------------------------------

def test_sval_ranks(sh, small):
    """Hits of rank 1 and of rank n_wish = 100 in one row (100 is also the
    largest n_wish of the packed wishlist context: n_wish % 4 == 0,
    n_wish <= 102), read by a first step and by a generic step."""
    sd, _ = small
    n = 70
    assert NW == 100
    order = np.random.default_rng(70).permutation(n)
    heads = [at_ranks([(order[j], NW), (order[j + 1], 1)]) for j in range(n - 1)]
    heads.append(at_ranks([(order[0], NW), (order[n - 1], 1)]))  # (column order[0] is row 0's by then)
    wish, types, rows = crafted(sd, order, heads)
    C = cost_v(wish[rows[0]], types[rows[0]])
    assert all(sorted(r[r < 0].tolist()) == [-NW * 512, -512] for r in C)
    T = sap_duals(C)
    assert any(len(d) > 1 for d in T["steps"])
    run(sh, sd, wish, types, rows)


def test_sval_marker_rows(sh, small):
    """Rows with more than 32 hits (entry 31 is the overflow marker): row 5 as
    a first-step row only; row 0, which first takes a column of its own, is
    read again by a generic step when row 200 wants that column alone."""
    sd, _ = small
    n = 256
    col_types = np.arange(n)
    held = np.random.default_rng(12).choice(np.arange(8, n), 40, replace=False)
    col_types[held] = NG - 1
    heads = [[] if j in held else [int(col_types[j])] for j in range(n)]
    heads[0] = [0, NG - 1]
    heads[5] = [NG - 1, 5]
    free = [int(j) for j in np.setdiff1d(np.arange(8, n), held)]
    heads[200] = [0]
    assert 200 not in held
    wish, types, rows = crafted(sd, col_types, heads)
    C = cost_v(wish[rows[0]], types[rows[0]])
    hits = (C < 0).sum(axis=1)
    assert hits[0] > 32 and hits[5] > 32 and (hits > 32).sum() == 2 and len(free) > 0
    assert int((hits[hits > 32] - 31).sum()) <= OVF_CAP
    T = sap_duals(C)
    assert [r for r, _, _, _ in T["steps"][0]] == [0] and [r for r, _, _, _ in T["steps"][5]] == [5]
    assert [r for r, _, _, _ in T["steps"][200]][:2] == [200, 0]
    run(sh, sd, wish, types, rows)


# -- the winner's lane mask --------------------------------------------------------------------

def test_winner_lanes(sh, small):
    """Generic steps whose winners sit in lanes 0, 31, 32 and 63 (columns 1,
    125, 130, 255 of a chain at n = 256), and a chain whose every winner is
    the column at the last position of `remaining` (pstar == last)."""
    sd, _ = small
    n, m = 256, 12
    rest = [int(x) for x in np.random.default_rng(5).permutation(n) if x not in (7, 1, 125, 130, 255)]
    order = np.array([7, 1, 125, 130, 255] + rest)
    cr = [int(x) for x in np.random.default_rng(6).choice(n - 1, m, replace=False)]
    wish, types, rows = chain(sd, n, order, cr)
    last = sap_duals(cost_v(wish[rows[0]], types[rows[0]]))["steps"][-1]
    assert len(last) == m + 1
    assert {j >> 2 for _, _, _, j in last[1:]} >= {0, 31, 32, 63}
    run(sh, sd, wish, types, rows)
    n2 = 133
    wish, types, rows = chain(sd, n2, np.arange(n2), list(range(m)))
    last = sap_duals(cost_v(wish[rows[0]], types[rows[0]]))["steps"][-1]
    assert len(last) == m + 1 and all(idx == nrem - 1 for _, idx, nrem, _ in last)
    run(sh, sd, wish, types, rows)
