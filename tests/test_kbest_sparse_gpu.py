"""The k best assignments on sparse (CSR) costs, on the GPU.

The contract is one sentence -- the sparse entries return what the dense ones
return for the densification -- so the yardsticks are existing code:

* lsap_murty_children_csr_ (murty_children_batched_sparse) against
  murty_children_batched on densify(...) with the same shapes and the same
  node: col and kept the same integers, cost the same bits, u and v equal by
  value (np.array_equal with NaN == NaN; a zero's sign is not compared, for the
  reason lsap_warm_csr_ documents).  Up to 65 columns every child also meets
  resolve_batched_sparse on its masked CSR written out by hand
  (kbest_sparse_families.masked_csr) and the host reference kbest_ref.child.
* lsap_kbest_csr_ (kbest_batched_sparse) against kbest_batched on the
  densification entry by entry (cols, count, the bits of costs), and up to 5
  rows against tests/kbest_ref.py.

Values are small integers stored as floats, so every order of summation gives
the same sum.  No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kbest_ref as KR  # noqa: E402
import kbest_sparse_families as KS  # noqa: E402
import lsap_sparse_families as S  # noqa: E402

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
INF = float("inf")


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("kbest_batched_sparse", "kbest_assignments_sparse", "murty_children_batched_sparse"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.array_equal(a, b, equal_nan=True)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


def words(F, NC):
    """A bool mask over the columns as the int64 words of the entries' bitmap."""
    b = np.zeros(((NC + 63) // 64) * 64, dtype=bool)
    b[:len(F)] = F
    return np.packbits(b, bitorder="little").view(np.int64)


def device_csr(bt, dtype):
    return (torch.from_numpy(bt.indptr).cuda(), torch.from_numpy(bt.indices).cuda(),
            torch.from_numpy(bt.data).to(TORCH[dtype]).cuda())


def dense_of(bt, dtype):
    """The padded densification as kbest_batched / murty_children_batched take it
    (what lies beyond a corner is never read: NaN there becomes +inf)."""
    D = np.where(np.isnan(bt.dense), np.inf, bt.dense)
    return torch.from_numpy(D).to(TORCH[dtype]).cuda()


# --------------------------------------------------------------------------- the expansion entry
PATTERNS = {"band": S.band_5pct, "word_edges": S.word_edges, "full": S.full}


@functools.lru_cache(maxsize=None)
def expansion_batch(pattern, nr, nc):
    """B = 3 instances of the pattern; instance 1 is ragged (entries stored beyond its corner)."""
    gen = PATTERNS[pattern]
    nr1 = max(1, nr - 2)
    nc1 = nc - 1 if nc - 1 >= nr1 else nc
    if pattern == "word_edges" and nc % 64 == 1 and nr < nc - 1:
        nc1 = nc  # (a row confined to the last word holds that word's one column: the corner keeps it)
    insts = []
    for seed, corner in ((0, (nr, nc)), (1, (nr1, nc1)), (2, (nr, nc))):
        g = gen(nr, nc, seed)
        P = np.isfinite(g.dense) if pattern != "full" else np.ones((nr, nc), dtype=bool)  # (full: +inf stays stored)
        insts.append(KS._inst(f"{pattern}{seed}", P, np.where(P, g.dense, 0) if pattern != "full" else g.dense, corner))
    return KS.batch(insts)


def forbidden_sets(stored, nc):
    """The six F of the cases, for a row p whose stored live columns are `stored`."""
    def mask(cols):
        F = np.zeros(nc, dtype=bool)
        F[list(cols)] = True
        return F
    absent = [j for j in range(nc) if j not in set(stored.tolist())]
    return (mask([]), mask(stored[len(stored) // 2:len(stored) // 2 + 1]), mask([min(63, nc - 1), min(64, nc - 1)]),
            mask(stored[:-1]), mask(stored), mask(absent[:1] if absent else [0]))


def run_children(sh, bt, dtype, pcol, pv, p, F, validate=True):
    """Both entries on one node per instance -> (sparse result, dense result) as host arrays."""
    B, NR, NC = bt.shape
    crow, idx, val = device_csr(bt, dtype)
    node = (torch.from_numpy(pcol.astype(np.int32)).cuda(), torch.from_numpy(pv).cuda(),
            torch.from_numpy(np.asarray(p, dtype=np.int32)).cuda(),
            torch.from_numpy(np.stack([words(f, NC) for f in F])).cuda())
    before = [a.clone() for a in (crow, idx, val) + node]
    got = sh.murty_children_batched_sparse(crow, idx, val, bt.shape, *node, shapes=bt.shapes, validate=validate)
    for a, b in zip((crow, idx, val) + node, before):
        assert bits(a) == bits(b), "an input was modified"
    col, cost, u, v, kept = got
    assert col.dtype == torch.int32 and kept.dtype == torch.int32 and cost.dtype == u.dtype == v.dtype == torch.float64
    assert tuple(col.shape) == (B, NR, NR) and tuple(cost.shape) == (B, NR) and tuple(u.shape) == (B, NR, NR)
    assert tuple(v.shape) == (B, NR, NC) and tuple(kept.shape) == (B, NR)
    want = sh.murty_children_batched(dense_of(bt, dtype), *node, shapes=bt.shapes)
    return [x.cpu().numpy() for x in got], [x.cpu().numpy() for x in want]


def assert_children_equal(got, want, where=()):
    col, cost, u, v, kept = got
    dcol, dcost, du, dv, dkept = want
    assert same(col, dcol), ("col",) + where
    assert same(kept, dkept), ("kept",) + where
    assert bits(cost) == bits(dcost), ("cost",) + where
    assert same(u, du), ("u",) + where
    assert same(v, dv), ("v",) + where


def instance_csr(bt, b):
    """Instance b's own CSR (NR rows) out of the batch."""
    NR = bt.shape[1]
    ip = bt.indptr[b * NR:(b + 1) * NR + 1]
    return ip - ip[0], bt.indices[ip[0]:ip[-1]], bt.data[ip[0]:ip[-1]]


def check_written_out(sh, bt, dtype, b, pcol, pv, p, F, got):
    """Every child of instance b against resolve_batched_sparse on its masked CSR
    written out, and against the host reference on the densification."""
    _, NR, NC = bt.shape
    nr, nc = int(bt.shapes[b][0]), int(bt.shapes[b][1])
    col, cost, u, v, kept = got
    exist = [t for t in range(NR) if 0 <= p <= t < nr]
    for t in set(range(NR)) - set(exist):  # no such child: -1, +inf, zero duals, kept 0
        assert (col[b, t] == -1).all() and cost[b, t] == INF and kept[b, t] == 0, (b, t)
        assert not u[b, t].any() and not v[b, t].any(), (b, t)
    if not exist:
        return
    ip, ix, va = instance_csr(bt, b)
    Cb = np.where(np.isnan(bt.dense[b]), np.inf, bt.dense[b])[:nr, :nc]
    cb = pcol[b].astype(np.int64)
    kids = [KS.masked_csr(ip, ix, va, cb, t, KR.forbidden_t(cb[:nr], p, F[:nc], t)) for t in exist]
    n = len(kids)
    base = np.concatenate([[0], np.cumsum([k[1].size for k in kids])])
    crow = np.concatenate([[0]] + [k[0][1:] + base[q] for q, k in enumerate(kids)]).astype(np.int64)
    rc, rcost, ru, rv, rkept = [x.cpu().numpy() for x in sh.resolve_batched_sparse(
        torch.from_numpy(crow).cuda(), torch.from_numpy(np.concatenate([k[1] for k in kids])).cuda(),
        torch.from_numpy(np.concatenate([k[2] for k in kids])).to(TORCH[dtype]).cuda(), (n, NR, NC),
        torch.from_numpy(np.tile(pcol[b], (n, 1)).astype(np.int32)).cuda(),
        torch.zeros((n, NR), dtype=torch.float64, device="cuda"), torch.from_numpy(np.tile(pv[b], (n, 1))).cuda(),
        shapes=np.tile([[nr, nc]], (n, 1)), validate=False)]
    for q, t in enumerate(exist):
        where = (b, t, p)
        assert same(col[b, t], rc[q]) and kept[b, t] == rkept[q], where
        assert same(u[b, t], ru[q]) and same(v[b, t], rv[q]), where
        if rc[q, 0] >= 0:
            assert bits(cost[b, t]) == bits(rcost[q]), where
        else:  # (an infeasible instance of the warm entries costs 0, an infeasible child +inf)
            assert cost[b, t] == INF and rcost[q] == 0, where
        ch = KR.child(Cb, cb[:nr], pv[b, :nc], p, F[:nc], t)
        if ch is None:
            assert (col[b, t] == -1).all() and cost[b, t] == INF, where
            assert np.isnan(u[b, t, :nr]).all() and np.isnan(v[b, t, :nc]).all(), where
        else:
            hc, hu, hv, hkept, _, _ = ch
            assert same(col[b, t, :nr], hc) and kept[b, t] == hkept, where
            assert same(u[b, t, :nr], hu) and same(v[b, t, :nc], hv), where
            assert cost[b, t] == Cb[np.arange(nr), hc].sum(), where


SIZES = (1, 2, 5, 64, 65, 256, 257, 512, 513, 1024)
EXPANSION = [(dt, nc - d, nc, pat) for dt in TORCH for nc in SIZES for d in (0, 3) if nc - d >= 1 for pat in PATTERNS]


@pytest.mark.parametrize("dtype,nr,nc,pattern", EXPANSION, ids=[f"{d}-{r}x{c}-{p}" for d, r, c, p in EXPANSION])
def test_children_against_the_dense_entry_on_the_densification(sh, dtype, nr, nc, pattern):
    bt = expansion_batch(pattern, nr, nc)
    B, NR, NC = bt.shape
    crow, idx, val = device_csr(bt, dtype)
    rcol, _, _, rv = sh.solve_batched_sparse(crow, idx, val, bt.shape, shapes=bt.shapes, duals=True)
    pcol, pv = rcol.cpu().numpy(), rv.cpu().numpy()
    assert (pcol[:2, 0] >= 0).all(), "the parents are feasible"
    nrs = [int(bt.shapes[b][0]) for b in range(B)]
    ps = [(0, n // 2, n - 1) for n in nrs]
    stored = lambda b, p: np.flatnonzero(np.isfinite(bt.dense[b, p, :bt.shapes[b][1]]))  # noqa: E731
    # call c: instance 0 gets (p_c, F kind c), the ragged instance 1 (p_{c+1}, F kind c + 3); instance 2 has no node
    for c in range(3):
        p0, p1 = ps[0][c], ps[1][(c + 1) % 3]
        F0 = forbidden_sets(stored(0, p0), NC)[c]
        F1 = forbidden_sets(stored(1, p1), NC)[c + 3]
        p, F = [p0, p1, -1], [F0, F1, np.zeros(NC, dtype=bool)]
        got, want = run_children(sh, bt, dtype, pcol, pv, p, F)
        assert_children_equal(got, want, (c,))
        assert (got[0][2] == -1).all() and (got[1][2] == INF).all() and not got[4][2].any()
        if c == 0 and pattern == "full" and nc >= 64:
            # p = 0, F empty, 3 % +inf: every child of instance 0 exists, but for the last one of a square
            # instance, whose last row is left its own column alone, which F_t closes
            live = nrs[0] - (nr == nc)
            assert (got[1][0, :live] < INF).all() and (got[0][0, :live, :nrs[0]] >= 0).all()
            assert nr != nc or got[1][0, nr - 1] == INF
        if c == 1:  # every stored column of row p1 is forbidden: that child is infeasible
            assert (got[0][1, p1] == -1).all() and got[1][1, p1] == INF
        if nc <= 65:
            for b in (0, 1):
                check_written_out(sh, bt, dtype, b, pcol, pv, p[b], F[b], got)


# --------------------------------------------------------------------------- the node is data
def garbage_batch(nr, nc):
    return band_batch(nr, nc, 3)


@pytest.mark.parametrize("dtype", TORCH)
@pytest.mark.parametrize("nr,nc", ((6, 6), (6, 9), (65, 65)))
def test_a_garbage_node_is_data(sh, dtype, nr, nc):
    rng = np.random.default_rng([5, nr, nc])
    bt = garbage_batch(nr, nc)
    B = 3
    pcol = rng.integers(-3, nc + 3, size=(B, nr))  # out of range and duplicated
    pcol[1] = rng.permutation(nc)[:nr]
    pcol[1, nr // 2] = pcol[1, 0]  # two forced rows on one column
    pv = rng.integers(-60, 20, size=(B, nc)).astype(np.float64)  # (positive values among them)
    pv[rng.random((B, nc)) < 0.2] = -np.inf
    pv[0, 0] = np.nan
    F = [rng.random(nc) < 0.3 for _ in range(B)]
    p = [0, 1, nr + 4]  # (p >= nr: no child)
    got, want = run_children(sh, bt, dtype, pcol, pv, p, F)
    assert_children_equal(got, want)
    assert (got[0][2] == -1).all() and (got[1][2] == INF).all()
    for b in (0, 1):
        check_written_out(sh, bt, dtype, b, pcol, pv, p[b], F[b], got)


@pytest.mark.parametrize("dtype", TORCH)
def test_a_forced_row_whose_column_is_not_stored_makes_the_child_infeasible(sh, dtype):
    bt = KS.batch([KS.tridiagonal(5)])
    pcol = np.array([[0, 3, 2, 1, 4]])  # (1, 3) and (3, 1) are not stored
    pv = np.zeros((1, 5))
    F = [np.zeros(5, dtype=bool)]
    got, want = run_children(sh, bt, dtype, pcol, pv, [0], F)
    assert_children_equal(got, want)
    col, cost = got[0], got[1]
    assert (col[0, 0, 0] >= 0) and (col[0, 1, 0] >= 0)  # rows 0 and 1 free: feasible (row 0 forced for t = 1)
    for t in (2, 3, 4):  # row 1 is forced to a column it does not store
        assert (col[0, t] == -1).all() and cost[0, t] == INF, t
    check_written_out(sh, bt, dtype, 0, pcol, pv, 0, F[0], got)


@pytest.mark.parametrize("dtype", TORCH)
def test_a_forced_chain_that_leaves_a_later_row_no_edge(sh, dtype):
    P = np.ones((5, 5), dtype=bool)
    P[3, 2:] = False  # row 3 stores columns 0 and 1, which rows 0 and 1 hold,
    P[3, 3] = True    # ... and column 3, its own: the root is feasible
    V = np.random.default_rng(13).integers(0, 50, size=(5, 5))
    bt = KS.batch([KS._inst("chain", P, V)])
    pcol, pv, F = np.array([[0, 1, 2, 3, 4]]), np.zeros((1, 5)), [np.zeros(5, dtype=bool)]
    got, want = run_children(sh, bt, dtype, pcol, pv, [0], F)
    assert_children_equal(got, want)
    # child 3 forbids (3, 3) and closes columns 0 .. 2 to row 3: no entry is left in it
    assert (got[0][0, 3] == -1).all() and got[1][0, 3] == INF and got[4][0, 3] == 0
    check_written_out(sh, bt, dtype, 0, pcol, pv, 0, F[0], got)


@pytest.mark.parametrize("dtype", TORCH)
def test_an_index_outside_the_live_columns_in_a_stored_tail_is_dropped(sh, dtype):
    # a ragged 3 x 4 corner of a 4 x 6 block; the rows' tails hold columns 4, 5 (beyond the corner) and 6, 9
    # (beyond the block): with validate=False they are read as data and never form an address
    rows = [[0, 1, 3, 5, 9], [0, 2, 4, 6], [1, 2, 3, 5], [0, 7]]
    vals = [[1, 2, 0, 7, 7], [3, 1, 7, 7], [0, 2, 2, 7], [7, 7]]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices, data = np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.float64)
    dense = np.full((1, 4, 6), np.inf)
    for i, (r, v) in enumerate(zip(rows, vals)):
        for j, x in zip(r, v):
            if j < 6:
                dense[0, i, j] = x
    bt = KS.Batch(indptr, indices, data, (1, 4, 6), np.array([[3, 4]], dtype=np.int32), dense)
    crow, idx, val = device_csr(bt, dtype)
    rcol, rcost, _, rv = sh.solve_batched_sparse(crow, idx, val, bt.shape, shapes=bt.shapes, duals=True, validate=False)
    assert rcol[0, 0] >= 0
    pcol, pv = rcol.cpu().numpy(), rv.cpu().numpy()
    for p in (0, 1):
        F = [np.zeros(6, dtype=bool)]
        F[0][[3, 5]] = p == 1
        got, want = run_children(sh, bt, dtype, pcol, pv, [p], F, validate=False)
        assert_children_equal(got, want, (p,))
    cols, costs, count = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=10, shapes=bt.shapes, validate=False)
    dcols, dcosts, dcount = sh.kbest_batched(dense_of(bt, dtype), 10, shapes=bt.shapes)
    assert same(cols, dcols) and bits(costs) == bits(dcosts) and same(count, dcount)
    assert int(count[0]) == 8  # (the corner's 3 x 4 pattern has eight assignments, by hand)


# --------------------------------------------------------------------------- the k best
def check_kbest(sh, bt, k, dtype="float64", maximize=False, reference=False):
    """kbest_batched_sparse on the batch against kbest_batched on its densification, entry by entry."""
    B, NR, NC = bt.shape
    crow, idx, val = device_csr(bt, dtype)
    before = [a.clone() for a in (crow, idx, val)]
    cols, costs, count = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=k, shapes=bt.shapes, maximize=maximize)
    for a, b in zip((crow, idx, val), before):
        assert bits(a) == bits(b), "an input was modified"
    assert cols.dtype == torch.int32 and costs.dtype == torch.float64 and count.dtype == torch.int32
    assert tuple(cols.shape) == (B, k, NR) and tuple(costs.shape) == (B, k) and tuple(count.shape) == (B,)
    D = dense_of(bt, dtype)
    if maximize:  # (a missing entry is forbidden whichever way the problem goes)
        D = torch.where(torch.isinf(D), -D, D)
    dcols, dcosts, dcount = sh.kbest_batched(D, k, shapes=bt.shapes, maximize=maximize)
    assert same(cols, dcols), "cols"
    assert same(count, dcount), "count"
    assert bits(costs) == bits(dcosts), "costs"
    cols, costs, count = cols.cpu().numpy(), costs.cpu().numpy(), count.cpu().numpy()
    if reference:
        for b in range(B):
            nr, nc = int(bt.shapes[b][0]), int(bt.shapes[b][1])
            if nr == 0:
                assert count[b] == 0 and (cols[b] == -1).all() and (costs[b] == INF).all(), b
                continue
            Cb = np.where(np.isnan(bt.dense[b]), np.inf, bt.dense[b])[:nr, :nc]
            rcols, rcosts, rcount, _, _ = KR.kbest(Cb, k)
            assert count[b] == rcount and same(cols[b, :, :nr], rcols) and (cols[b, :, nr:] == -1).all(), b
            assert bits(costs[b]) == bits(rcosts), b
    return cols, costs, count


def test_kbest_small_family_batched_and_ragged_in_one_call(sh):
    bt = KS.batch(KS.family())
    for dtype in TORCH:
        _, _, count = check_kbest(sh, bt, KS.K, dtype=dtype, reference=dtype == "float64")
        assert (count == 0).any() and ((count > 0) & (count < KS.K)).any() and (count == KS.K).any()


def tridiagonal8():
    i = np.arange(8)
    return KS._inst("tridiagonal8", np.abs(i[:, None] - i[None, :]) <= 1, (i[:, None] + i[None, :]) % 2)


@pytest.mark.parametrize("dtype", TORCH)
def test_kbest_runs_into_the_tail(sh, dtype):
    _, costs, count = check_kbest(sh, KS.batch([tridiagonal8(), KS.bidiagonal4()]), 40, dtype=dtype)
    assert count.tolist() == [34, 1]  # F(9) perfect matchings of the tridiagonal 8 x 8, one of the bidiagonal
    assert (np.diff(costs[0, :34]) >= 0).all() and (costs[0, 34:] == INF).all() and (costs[1, 1:] == INF).all()


@functools.lru_cache(maxsize=None)
def band_batch(nr, nc, B):
    insts = []
    for q in range(B):
        g = S.band_40pct(nr, nc, q)
        P = np.isfinite(g.dense)
        insts.append(KS._inst(f"band{q}", P, np.where(P, g.dense, 0)))
    return KS.batch(insts)


@functools.lru_cache(maxsize=None)
def host_trace(nr, nc, b, k):
    return KR.kbest(band_batch(nr, nc, 2 if nc < 200 else 1).dense[b], k)


def certify_ranks(sh, dtype, bt, b, k, cols):
    """Each emitted assignment with the duals the GPU ends its node with, on the
    node's masked CSR written out: check_duals_sparse says 0."""
    _, nr, nc = bt.shape
    rcols, _, rcount, _, trace = host_trace(nr, nc, b, k)
    assert rcount == k and same(cols[b], rcols)
    ip, ix, va = instance_csr(bt, b)
    one = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).cuda() if dt is None \
        else torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()  # noqa: E731
    for r, origin in enumerate(trace):
        if origin is None:
            csr = (ip, ix, va)
            col, _, u, v = sh.solve_batched_sparse(one(ip), one(ix), one(va, TORCH[dtype]), (1, nr, nc), duals=True)
        else:
            pcol, pv, p, F, t = origin
            ccol, _, cu, cv, _ = sh.murty_children_batched_sparse(
                one(ip), one(ix), one(va, TORCH[dtype]), (1, nr, nc), one(pcol.astype(np.int32))[None], one(pv)[None],
                torch.tensor([p], dtype=torch.int32, device="cuda"), one(words(F, nc))[None])
            col, u, v = ccol[:, t].contiguous(), cu[:, t].contiguous(), cv[:, t].contiguous()
            csr = KS.masked_csr(ip, ix, va, pcol, t, KR.forbidden_t(pcol, p, F, t))
        assert same(col[0], rcols[r]), r
        _, flags = sh.check_duals_sparse(one(csr[0]), one(csr[1]), one(csr[2], TORCH[dtype]), (1, nr, nc), col, u, v)
        assert flags.cpu().tolist() == [0], r


KBEST = [("float64", 65, 65, 3), ("float32", 65, 65, 3), ("float64", 60, 67, 3), ("float32", 60, 67, 3),
         ("float64", 257, 257, 2), ("float32", 257, 257, 2)]


@pytest.mark.parametrize("dtype,nr,nc,k", KBEST, ids=[f"{d}-{r}x{c}-k{k}" for d, r, c, k in KBEST])
def test_kbest_against_the_dense_entry_and_certified(sh, dtype, nr, nc, k):
    bt = band_batch(nr, nc, 2 if nc < 200 else 1)
    cols, costs, count = check_kbest(sh, bt, k, dtype=dtype)
    assert (count == k).all() and (np.diff(costs, axis=1) >= 0).all()
    if nc in (65, 257):
        for b in range(bt.shape[0]):
            certify_ranks(sh, dtype, bt, b, k, cols)


def test_maximize_negates_the_problem(sh):
    bt = KS.batch([g for g in KS.family() if not np.isinf(g.data).any()])  # (under maximize +inf is no entry's value)
    cols, costs, count = check_kbest(sh, bt, 9, maximize=True)
    crow, idx, val = device_csr(bt, "float64")
    mcols, mcosts, mcount = sh.kbest_batched_sparse(crow, idx, -val, bt.shape, k=9, shapes=bt.shapes)
    assert same(cols, mcols) and same(costs, -mcosts.cpu().numpy()) and same(count, mcount)
    assert (costs[count == 0] == -INF).all() and (count == 0).any()  # exhausted ranks read -inf


@pytest.mark.parametrize("dtype", TORCH)
def test_k_one_is_the_sparse_solve_bit_for_bit(sh, dtype):
    for bt in (KS.batch(KS.family()), band_batch(65, 65, 2), band_batch(60, 67, 2), band_batch(257, 257, 1)):
        crow, idx, val = device_csr(bt, dtype)
        cols, costs, count = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=1, shapes=bt.shapes)
        col, cost = sh.solve_batched_sparse(crow, idx, val, bt.shape, shapes=bt.shapes)
        ok = col[:, 0] >= 0
        assert torch.equal(cols[:, 0], col) and torch.equal(count, ok.to(torch.int32))
        assert bits(costs[ok, 0]) == bits(cost[ok]) and bool((costs[~ok, 0] == INF).all())


def test_an_infeasible_root_and_a_batch_without_entries(sh):
    by_name = {g.name: g for g in KS.family()}
    bt = KS.batch([by_name["hall"], by_name["tridiagonal3"], by_name["empty_row"]])
    cols, costs, count = check_kbest(sh, bt, 4)
    assert count.tolist() == [0, 3, 0] and (cols[[0, 2]] == -1).all() and (costs[[0, 2]] == INF).all()
    B, NR, NC = 3, 4, 70
    crow = torch.zeros(B * NR + 1, dtype=torch.int64, device="cuda")
    for dt in TORCH.values():
        cols, costs, count = sh.kbest_batched_sparse(crow, torch.zeros(0, dtype=torch.int32, device="cuda"),
                                                     torch.zeros(0, dtype=dt, device="cuda"), (B, NR, NC), k=3)
        assert bool((cols == -1).all()) and bool((costs == INF).all()) and not count.any()
        assert tuple(cols.shape) == (B, 3, NR)


def test_kbest_is_deterministic(sh):
    bt = band_batch(60, 67, 2)
    crow, idx, val = device_csr(bt, "float64")
    a = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=12)
    b = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=12)
    for x, y in zip(a, b):
        assert bits(x) == bits(y)


def test_a_sparse_csr_tensor_in_place_of_the_triple(sh):
    bt = KS.batch([g for g in KS.family() if g.corner == g.shape and g.shape[0]])
    crow, idx, val = device_csr(bt, "float64")
    B, NR, NC = bt.shape
    A = torch.sparse_csr_tensor(crow, idx.long(), val, size=(B * NR, NC))
    a = sh.kbest_batched_sparse(A, shape=bt.shape, k=5, shapes=bt.shapes)
    b = sh.kbest_batched_sparse(crow, idx, val, bt.shape, k=5, shapes=bt.shapes)
    for x, y in zip(a, b):
        assert bits(x) == bits(y)


# --------------------------------------------------------------------------- the single-matrix front end
def test_kbest_assignments_sparse_on_a_scipy_matrix_and_on_a_tall_one(sh):
    sp = pytest.importorskip("scipy.sparse")
    g = S.band_40pct(9, 12, 3)
    P = np.isfinite(g.dense)
    for D in (g.dense, g.dense.T):  # wide, and tall: solved as its transpose
        Pm = np.isfinite(D)
        A = sp.csr_matrix((D[Pm], np.nonzero(Pm)[1], np.concatenate([[0], np.cumsum(Pm.sum(1))])), shape=D.shape)
        for maximize in (False, True):
            cols, costs = sh.kbest_assignments_sparse(A, 7, maximize=maximize)
            dcols, dcosts = sh.kbest_assignments(np.where(Pm, D, -INF if maximize else INF), 7, maximize=maximize)
            assert cols.dtype == np.int64 and cols.shape == (7, D.shape[0]) and same(cols, dcols)
            assert bits(costs) == bits(dcosts)
    assert P.sum() < P.size
    ip, ix, va = S.csr_of(P, np.where(P, g.dense, 0))
    cols, costs = sh.kbest_assignments_sparse((ip, ix, va.astype(np.float32), g.dense.shape), 4)
    dcols, dcosts = sh.kbest_assignments(g.dense.astype(np.float32), 4)
    assert same(cols, dcols) and bits(costs) == bits(dcosts)
    none = sh.kbest_assignments_sparse((np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (3, 3)), 2)
    assert none[0].shape == (0, 3) and none[1].shape == (0,)
