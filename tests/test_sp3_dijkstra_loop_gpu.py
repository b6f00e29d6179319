"""santa_sp3_kernel's Dijkstra loop: the inner loop of
consecutive single-step Dijkstras and its exits into and returns from the
multi-step path, the two halves of the register tile, and the book-keeping of
`remaining` (winner, mover) -- on crafted blocks, in the pattern of
test_sp3_first_step_gpu.py.

Every case first asserts on the CPU (lsap_families.sap_trace, and sap_steps
below, which is checked against it) the property that makes it meaningful;
then the sparse kernel (SH_FLAG_SP_TILE) must equal the oracle's round: col,
exact cost, per-block steps, the new type vector and the happiness deltas.

(The first Dijkstra of a block cannot be multi-step -- no column is assigned
yet, so its first scan always ends at an unassigned one -- hence the earliest
multi-step Dijkstra a block can have is its second: test_back_edges[second_multi].)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from lsap_families import sap_trace  # noqa: E402
from test_sp3_first_step_gpu import (FILL0, NG, check_blocks, cost_v, crafted, dijkstra_lengths,  # noqa: E402,F401
                                     sh, small, small_ctx)

pytestmark = pytest.mark.gpu


def sap_steps(C):
    """scipy's solve as sap_trace runs it, recording per Dijkstra its steps as
    (row, position of the winner in `remaining`, len(remaining), winner)."""
    C = np.ascontiguousarray(C, dtype=np.int64)
    nr, nc = C.shape
    INF = np.iinfo(np.int64).max
    u, v = np.zeros(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64)
    path = -np.ones(nc, dtype=np.int64)
    col4row, row4col = -np.ones(nr, dtype=np.int64), -np.ones(nc, dtype=np.int64)
    out = []
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1)
        spc = np.full(nc, INF, dtype=np.int64)
        SR, SC, rec = [], [], []
        minVal, i = 0, cur
        while True:
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
        out.append(rec)
    assert np.array_equal(col4row, sap_trace(C)[0])
    return out


def run(sh, sd, wish, types, rows):
    from santa_hip import _lib
    c = small_ctx(sh, sd, wish)
    steps = check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE)
    c.close()
    return steps


M = 40  # rows of a chain: each hop costs one rank (512), so a path of up to ~100 hops beats a miss


def chain(sd, n, order, cr):
    """The rows cr[t] want column order[t], then order[t + 1]; the last row
    wants order[0] only; every other row wants a column of its own: n - 1
    single-step Dijkstras, then one whose path shifts every row of cr
    (len(cr) + 1 steps and hops)."""
    m = len(cr)
    assert n - 1 not in cr and len(set(cr)) == m
    heads = [None] * n
    for t, r in enumerate(cr):
        heads[r] = [int(order[t]), int(order[t + 1])]
    heads[n - 1] = [int(order[0])]
    own = iter(order[m + 1:])
    heads = [h if h is not None else [int(next(own))] for h in heads]
    return crafted(sd, np.arange(n), heads)


def classes(rows_):
    return {(int(i) & 1, (int(i) >> 1) & 1) for i in rows_}


# -- the tile's halves (rows below and from 128) ------------------------------------------

@pytest.mark.parametrize("n", [130, 256, 128])
def test_tile_halves(sh, small, n):
    """The last Dijkstra's path runs through rows on both sides of 128 at
    n = 130 and 256 (tile registers T0 and T1), in both 16-bit halves of a
    tile dword (i & 1) and both halves of the wave ((i >> 1) & 1), as far as
    the rows from 128 on have them; n = 128 is the control that uses T0 only.
    The columns lie anywhere in the lanes."""
    sd, _ = small
    rng = np.random.default_rng(n)
    order = rng.permutation(n)
    hi = list(range(128, min(n - 1, 132))) + list(rng.choice(np.arange(132, max(n - 1, 133)), 16, replace=False)
                                                  if n - 1 > 148 else [])
    lo = [0, 1, 2, 3] + list(rng.choice(np.arange(4, 127), M - 4 - len(hi), replace=False))
    cr = [int(x) for x in rng.permutation(lo + hi)]
    wish, types, rows = chain(sd, n, order, cr)
    C = cost_v(wish[rows[0]], types[rows[0]])
    S, longest = dijkstra_lengths(C)
    assert (S[:-1] == 1).all() and S[-1] == M + 1 and longest == M + 1
    seen = np.array([i for i, _, _, _ in sap_steps(C)[-1]])
    assert sorted(seen) == sorted(cr + [n - 1])
    assert classes(seen[seen < 128]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert classes(seen[seen >= 128]) == classes(range(128, min(n, 132)))
    assert (n > 128) == bool((seen >= 128).sum() >= 2)
    assert run(sh, sd, wish, types, rows).tolist() == [n + M]


# -- `remaining`: the winner's position and the mover --------------------------------------

def test_all_miss(sh, small):
    """Every cost is equal (no row wishes a type of the block): every decision
    is the order of `remaining` -- the last unassigned column of the scan."""
    sd, _ = small
    n = 131
    wish, types, rows = crafted(sd, np.arange(n), [[] for _ in range(n)])
    C = cost_v(wish[rows[0]], types[rows[0]])
    assert (C == 1).all()
    st = sap_steps(C)
    assert all(len(d) == 1 for d in st)
    assert [d[0][3] for d in st] == list(range(n))  # (column 0 is the scan's last)
    run(sh, sd, wish, types, rows)


def test_popular_type(sh, small):
    """One gift type on 31 columns, the first wish of the rows that take them
    and of the last 32 rows, whose second wish -- a column of their own, 32
    hits with it: the most a row holds without the overflow list -- stands one
    rank lower from row to row, so that the popular columns stay strictly
    better: each of the last 32 Dijkstras visits all 31 before it ends."""
    sd, _ = small
    n, k = 256, 31
    col_types = np.arange(n)
    held = np.sort(np.random.default_rng(23).choice(n, k, replace=False))
    col_types[held] = NG - 1
    free = [int(j) for j in np.setdiff1d(np.arange(n), held)]  # (their types are their indices)
    heads = [[NG - 1] for _ in range(k)] + [[c] for c in free[:n - k - 32]]
    for t, c in enumerate(free[n - k - 32:]):
        heads.append([NG - 1] + list(range(FILL0, FILL0 + t + 1)) + [c])
    wish, types, rows = crafted(sd, col_types, heads)
    C = cost_v(wish[rows[0]], types[rows[0]])
    assert ((C < 0).sum(axis=1) <= 32).all() and ((C[-32:] < 0).sum(axis=1) == 32).all()
    S, _ = dijkstra_lengths(C)
    assert (S[:-32] == 1).all() and (S[-32:] == 32).all()
    run(sh, sd, wish, types, rows)


@pytest.mark.parametrize("identity", [True, False])
def test_winner_last_and_mover_zero(sh, small, identity):
    """The chain over rows 0 .. M - 1 with the columns in row order: the
    multi-step Dijkstra's winners are columns 0, 1, ..., each at the last
    position of `remaining` when it wins (pstar == last at the hand-over and
    at every later step: the move is a no-op).  With rows and columns permuted
    the hand-over's winner is not column 0, so column 0 -- the last of a
    pristine `remaining` -- is the mover after the hand-over, and later steps
    move other columns."""
    sd, _ = small
    n = 133
    rng = np.random.default_rng(7)
    order = np.arange(n) if identity else rng.permutation(n)
    if not identity and order[0] == 0:
        order[[0, 1]] = order[[1, 0]]
    cr = list(range(M)) if identity else [int(x) for x in rng.choice(n - 1, M, replace=False)]
    wish, types, rows = chain(sd, n, order, cr)
    C = cost_v(wish[rows[0]], types[rows[0]])
    last = sap_steps(C)[-1]
    assert len(last) == M + 1
    at_last = [idx == nrem - 1 for _, idx, nrem, _ in last]
    if identity:
        assert all(at_last) and last[0][3] == 0
    else:
        assert not at_last[0] and last[0][3] != 0  # the hand-over moves column 0 to the winner's place
        assert not all(at_last[1:])
    run(sh, sd, wish, types, rows)


# -- the loop's back edges -------------------------------------------------------------------

def runs_block(sd, n, kinds):
    """Row j of kind 1 wants its own column (a single-step Dijkstra); of kind
    2 the column of row j - 1 first and its own second (the first scan ends at
    an assigned column)."""
    order = np.random.default_rng(n).permutation(n)
    heads = [[int(order[j])] if k == 1 else [int(order[j - 1]), int(order[j])] for j, k in enumerate(kinds)]
    return crafted(sd, order, heads)


@pytest.mark.parametrize("pattern", ["single_runs", "multi_runs", "second_multi", "alternate"])
def test_back_edges(sh, small, pattern):
    """Runs of single-step Dijkstras (1, 2, 3, 5, 8 long) each followed by a
    multi-step one; the reverse (runs of multi-step ones, a single-step one
    between); a block whose second Dijkstra is multi-step (the inner loop is
    left after one pass); strict alternation up to the block's last Dijkstra."""
    sd, _ = small
    n = 139
    if pattern == "single_runs":
        kinds = [k for _, r in zip(range(n), np.tile([1, 2, 3, 5, 8], n)) for k in [1] * r + [2]][:n]
    elif pattern == "multi_runs":
        kinds = [1] + [k for _, r in zip(range(n), np.tile([1, 2, 3, 5, 8], n)) for k in [2] * r + [1]][:n - 1]
    elif pattern == "second_multi":
        kinds = [1, 2] + [1] * (n - 2)
    else:
        kinds = [1 + (j & 1) for j in range(n)]
        assert kinds[-1] == 1 and kinds[-2] == 2
    wish, types, rows = runs_block(sd, n, kinds)
    S, _ = dijkstra_lengths(cost_v(wish[rows[0]], types[rows[0]]))
    assert len(S) == n and ((S == 1) == (np.asarray(kinds) == 1)).all()
    run(sh, sd, wish, types, rows)


def test_only_single_step_then_one_multi_at_the_end(sh, small):
    """Only single-step Dijkstras (the kernel never leaves the inner loop), at
    an n that is no multiple of four; and the same block with the last row's
    Dijkstra multi-step (the outer loop ends right after the augmentation)."""
    sd, _ = small
    n = 201
    for kinds in ([1] * n, [1] * (n - 1) + [2]):
        wish, types, rows = runs_block(sd, n, kinds)
        S, _ = dijkstra_lengths(cost_v(wish[rows[0]], types[rows[0]]))
        assert ((S == 1) == (np.asarray(kinds) == 1)).all()
        run(sh, sd, wish, types, rows)
