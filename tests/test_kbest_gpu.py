"""The k best assignments on the GPU.

* lsap_murty_children_ (murty_children_batched) against two oracles that
  already exist: resolve_batched on the materialised masked matrix M_t (col,
  kept and cost equal as bits, u and v by value), and, up to 65 columns, the
  host reference lsap_warm_ref.warm on the same matrix.  Above 65 columns a
  handful of children per instance meets resolve_batched and every other one
  is checked for what any child must satisfy.
* lsap_kbest_ (kbest_batched) against tests/kbest_ref.py entry by entry.

Costs are integers below 2^20 stored as floats, so every order of summation
gives the same sum and costs compare as bits; one case of generic floats
checks validity, order and the rounding bound of the cost alone.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kbest_families as KF  # noqa: E402
import kbest_ref as KR  # noqa: E402
import lsap_warm_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
INF = float("inf")


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("kbest_batched", "kbest_assignments", "murty_children_batched"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def words(F, NC):
    """A bool mask over the columns as the int64 words of the entries' bitmap."""
    bits = np.zeros(((NC + 63) // 64) * 64, dtype=bool)
    bits[:len(F)] = F
    return np.packbits(bits, bitorder="little").view(np.int64)


def costs(B, nr, nc, seed, hi=1 << 20):
    return np.random.default_rng([seed, nr, nc]).integers(0, hi, size=(B, nr, nc)).astype(np.float64)


# --------------------------------------------------------------------------- the expansion entry
def expand(sh, Ct, shapes, pcol, pv, p, F):
    """murty_children_batched on host arrays -> host arrays; the inputs must come back unchanged."""
    B, NR, NC = Ct.shape
    args = (torch.from_numpy(pcol.astype(np.int32)).cuda(), torch.from_numpy(pv).cuda(),
            torch.from_numpy(np.asarray(p, dtype=np.int32)).cuda(),
            torch.from_numpy(np.stack([words(f, NC) for f in F])).cuda())
    before = [a.clone() for a in args] + [Ct.clone()]
    out = sh.murty_children_batched(Ct, *args, shapes=shapes)
    for a, b in zip(list(args) + [Ct], before):
        assert same(a.cpu().numpy(), b.cpu().numpy()), "inputs were modified"
    col, cost, u, v, kept = out
    assert col.dtype == torch.int32 and kept.dtype == torch.int32 and cost.dtype == u.dtype == v.dtype == torch.float64
    assert tuple(col.shape) == (B, NR, NR) and tuple(cost.shape) == (B, NR) and tuple(u.shape) == (B, NR, NR)
    assert tuple(v.shape) == (B, NR, NC) and tuple(kept.shape) == (B, NR)
    return [x.cpu().numpy() for x in out]


def check_children(sh, Ct, shapes, pcol, pv, p, F, parent_cost, every):
    """One call of the entry, checked: `every` compares every child with both
    oracles, otherwise the children {p, p+1, 63, 64, nr-1} meet resolve_batched
    and the rest the properties of any child."""
    B, NR, NC = Ct.shape
    Ch = Ct.double().cpu().numpy()
    col, cost, u, v, kept = expand(sh, Ct, shapes, pcol, pv, p, F)
    for b in range(B):
        nr, nc = (NR, NC) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        pb = int(p[b])
        exist = [t for t in range(NR) if pb >= 0 and pb <= t < nr]
        for t in set(range(NR)) - set(exist):  # no such child: -1, +inf, zero duals, kept 0
            assert (col[b, t] == -1).all() and cost[b, t] == INF and kept[b, t] == 0, (b, t)
            assert not u[b, t].any() and not v[b, t].any(), (b, t)
        if not exist:
            continue
        Cb, cb, vb = Ch[b, :nr, :nc], pcol[b, :nr].astype(np.int64), pv[b, :nc]
        full = exist if every else sorted({t for t in (pb, pb + 1, 63, 64, nr - 1) if t in exist})
        Ms = {t: KR.masked(Cb, cb, t, KR.forbidden_t(cb, pb, F[b][:nc], t)) for t in full}
        # resolve_batched on the materialised matrices, one padded batch
        pad = np.zeros((len(full), NR, NC))
        for q, t in enumerate(full):
            pad[q, :nr, :nc] = Ms[t]
        n = len(full)
        rc, rcost, ru, rv, rkept = [x.cpu().numpy() for x in sh.resolve_batched(
            torch.from_numpy(pad).to(Ct.dtype).cuda(), torch.from_numpy(np.tile(pcol[b], (n, 1)).astype(np.int32)).cuda(),
            torch.zeros((n, NR), dtype=torch.float64, device="cuda"), torch.from_numpy(np.tile(pv[b], (n, 1))).cuda(),
            shapes=np.tile([[nr, nc]], (n, 1)))]
        for q, t in enumerate(full):
            where = (b, t, pb)
            assert same(col[b, t], rc[q]), where
            assert kept[b, t] == rkept[q], where
            assert same(u[b, t], ru[q]) and same(v[b, t], rv[q]), where
            if rc[q, 0] >= 0:
                assert cost[b, t].tobytes() == rcost[q].tobytes(), where
            else:  # (an infeasible instance of the warm entries costs 0, an infeasible child +inf)
                assert cost[b, t] == INF and rcost[q] == 0, where
            if every:
                try:
                    hc, hu, hv, hkept, searches = W.warm(Ms[t], cb, vb)
                    assert searches == nr - hkept, where
                    assert same(col[b, t, :nr], hc) and kept[b, t] == hkept, where
                    assert same(u[b, t, :nr], hu) and same(v[b, t, :nc], hv), where
                    assert cost[b, t] == Cb[np.arange(nr), hc].sum(), where
                except ValueError:
                    assert (col[b, t] == -1).all() and cost[b, t] == INF, where
                    assert np.isnan(u[b, t, :nr]).all() and np.isnan(v[b, t, :nc]).all(), where
        for t in set(exist) - set(full):  # what any child of a valid node satisfies
            ct = col[b, t, :nr].astype(np.int64)
            where = (b, t, pb)
            if ct[0] < 0:
                assert (ct == -1).all() and cost[b, t] == INF, where
                continue
            assert same(ct[:t], cb[:t]), where
            assert not KR.forbidden_t(cb, pb, F[b][:nc], t)[ct[t]], where
            assert ((ct >= 0) & (ct < nc)).all() and np.unique(ct).size == nr, where
            assert (col[b, t, nr:] == -1).all(), where
            assert cost[b, t] == Cb[np.arange(nr), ct].sum() and cost[b, t] >= parent_cost[b], where
    return col, cost


def scenario_masks(nc, nc1):
    """The forbidden sets of the cases, over the live columns of instance 0 (nc) and 1 (nc1)."""
    one = np.zeros(nc1, dtype=bool)
    one[nc1 // 2] = True
    seam = np.zeros(nc, dtype=bool)
    seam[[min(63, nc - 1), min(64, nc - 1)]] = True  # bits 63 and 64: the word seam
    but_one = np.ones(nc1, dtype=bool)
    but_one[nc1 - 1] = False
    return one, seam, but_one


SIZES = (1, 2, 5, 64, 65, 256, 257, 512, 513, 1024)
EXPANSION = [(dt, nc - d, nc) for dt in TORCH for nc in SIZES for d in (0, 3) if nc - d >= 1]


@pytest.mark.parametrize("dtype,nr,nc", EXPANSION, ids=[f"{d}-{r}x{c}" for d, r, c in EXPANSION])
def test_children_against_resolve_batched_and_the_host_reference(sh, dtype, nr, nc):
    B = 3
    Ct = torch.from_numpy(costs(B, nr, nc, 11)).to(TORCH[dtype]).cuda()
    nr1 = max(1, nr - 2)
    nc1 = nc - 1 if nc - 1 >= nr1 else nc
    shapes = np.array([[nr, nc], [nr1, nc1], [nr, nc]])
    rcol, rcost, _, rv = sh.solve_batched_large(Ct, shapes=shapes, duals=True)
    pcol, pv, parent_cost = rcol.cpu().numpy(), rv.cpu().numpy(), rcost.cpu().numpy()
    one, seam, but_one = scenario_masks(nc, nc1)
    none0, none2 = np.zeros(nc, dtype=bool), np.zeros(nc, dtype=bool)
    pad = lambda f: np.concatenate([f, np.zeros(nc - len(f), dtype=bool)])  # noqa: E731
    every = nc <= 65
    # (p of instance 0, F of 0, p of the ragged instance 1, F of 1); instance 2 has no node
    cases = ((0, none0, nr1 // 2, one), (nr // 2, seam, nr1 - 1, but_one), (nr - 1, np.ones(nc, dtype=bool), 0, one))
    for p0, F0, p1, F1 in cases:
        col, cost = check_children(sh, Ct, shapes, pcol, pv, [p0, p1, -1], [F0, pad(F1), none2], parent_cost, every)
        if F0.all():  # every live column forbidden in row p: that child is infeasible
            assert (col[0, p0] == -1).all() and cost[0, p0] == INF


@pytest.mark.parametrize("dtype", TORCH)
@pytest.mark.parametrize("nr,nc", ((6, 6), (6, 9), (65, 65)))
def test_a_garbage_node_is_data(sh, dtype, nr, nc):
    rng = np.random.default_rng([5, nr, nc])
    B = 3
    Ct = torch.from_numpy(costs(B, nr, nc, 12, hi=50)).to(TORCH[dtype]).cuda()
    pcol = rng.integers(-3, nc + 3, size=(B, nr))  # out of range and duplicated
    pcol[1] = rng.permutation(nc)[:nr]
    pcol[1, nr // 2] = pcol[1, 0]  # two forced rows on one column
    pv = rng.integers(-60, 20, size=(B, nc)).astype(np.float64)
    pv[rng.random((B, nc)) < 0.2] = -np.inf
    pv[0, 0] = np.nan
    F = [rng.random(nc) < 0.3 for _ in range(B)]
    check_children(sh, Ct, None, pcol, pv, [0, 1, nr + 4], F, np.full(B, -INF), True)


@pytest.mark.parametrize("dtype", TORCH)
def test_a_forced_chain_that_leaves_a_later_row_nothing_is_infeasible_in_the_prologue(sh, dtype):
    nr = nc = 5
    C = costs(1, nr, nc, 13, hi=50)
    C[0, 3, 2:] = np.inf  # row 3 can only take columns 0 and 1, which rows 0 and 1 hold
    C[0, 3, 3] = 7.0      # ... and column 3, its own: the root is feasible
    Ct = torch.from_numpy(C).to(TORCH[dtype]).cuda()
    pcol = np.array([[0, 1, 2, 3, 4]])
    pv = np.zeros((1, nc))
    F = [np.zeros(nc, dtype=bool)]
    col, cost = check_children(sh, Ct, None, pcol, pv, [0], F, np.full(1, -INF), True)
    # child 3 forbids (3, 3) and closes columns 0 .. 2 to row 3: nothing finite is left in it
    assert (col[0, 3] == -1).all() and cost[0, 3] == INF
    _, _, _, _, kept = sh.murty_children_batched(
        Ct, torch.from_numpy(pcol.astype(np.int32)).cuda(), torch.from_numpy(pv).cuda(),
        torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros((1, 1), dtype=torch.int64, device="cuda"))
    assert kept[0, 3] == 0


# --------------------------------------------------------------------------- the k best
def check_kbest(sh, Ch, k, dtype="float64", shapes=None, certify=False):
    """kbest_batched on the padded host batch Ch against the reference, entry by entry."""
    B, NR, NC = Ch.shape
    Ct = torch.from_numpy(Ch).to(TORCH[dtype]).cuda()
    before = Ct.clone()
    cols, cost, count = sh.kbest_batched(Ct, k, shapes=shapes)
    assert same(Ct.cpu().numpy(), before.cpu().numpy()), "inputs were modified"
    assert cols.dtype == torch.int32 and cost.dtype == torch.float64 and count.dtype == torch.int32
    assert tuple(cols.shape) == (B, k, NR) and tuple(cost.shape) == (B, k) and tuple(count.shape) == (B,)
    cols, cost, count = cols.cpu().numpy(), cost.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        nr, nc = (NR, NC) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        Cb = Ct[b, :nr, :nc].double().cpu().numpy()
        if nr == 0:
            assert count[b] == 0 and (cols[b] == -1).all() and (cost[b] == INF).all(), b
            continue
        rcols, rcost, rcount, _, trace = KR.kbest(Cb, k)
        assert count[b] == rcount, b
        assert same(cols[b, :, :nr], rcols) and (cols[b, :, nr:] == -1).all(), b
        assert cost[b].tobytes() == rcost.tobytes(), b
        if certify:
            certify_ranks(sh, Ct.dtype, Cb, rcols, trace)
    return cols, cost, count


def certify_ranks(sh, dtype, Cb, rcols, trace):
    """Each emitted assignment with the duals the GPU ends its node with, on the
    node's materialised matrix: check_duals_large says 0."""
    nr, nc = Cb.shape
    Ct = torch.from_numpy(Cb).to(dtype).cuda()[None]
    for r, origin in enumerate(trace):
        if origin is None:
            M = Ct
            col, _, u, v = sh.solve_batched_large(Ct, duals=True)
        else:
            pcol, pv, p, F, t = origin
            ccol, _, cu, cv, _ = sh.murty_children_batched(
                Ct, torch.from_numpy(pcol.astype(np.int32)).cuda()[None], torch.from_numpy(pv).cuda()[None],
                torch.tensor([p], dtype=torch.int32, device="cuda"), torch.from_numpy(words(F, nc)).cuda()[None])
            col, u, v = ccol[:, t], cu[:, t], cv[:, t]
            M = torch.from_numpy(KR.masked(Cb, pcol, t, KR.forbidden_t(pcol, p, F, t))).to(dtype).cuda()[None]
        assert same(col[0].cpu().numpy(), rcols[r]), r
        assert sh.check_duals_large(M, col.contiguous(), u.contiguous(), v.contiguous())[3].cpu().tolist() == [0], r


def test_kbest_small_family_batched_and_ragged_in_one_call(sh):
    fam = KF.small_family()
    NR, NC = max(C.shape[0] for C in fam), max(C.shape[1] for C in fam)
    Ch = np.full((len(fam), NR, NC), 3.0)  # (the padding is never read)
    for b, C in enumerate(fam):
        Ch[b, :C.shape[0], :C.shape[1]] = C
    shapes = np.array([C.shape for C in fam])
    _, _, count = check_kbest(sh, Ch, KF.K_SMALL, shapes=shapes)
    assert (count == 0).any() and ((count > 0) & (count < KF.K_SMALL)).any() and (count == KF.K_SMALL).any()


KBEST = [("float64", 8, 8, 30), ("float32", 8, 8, 30), ("float64", 65, 65, 3), ("float64", 60, 67, 3),
         ("float32", 60, 67, 3), ("float64", 257, 257, 2), ("float32", 257, 257, 2)]


@pytest.mark.parametrize("dtype,nr,nc,k", KBEST, ids=[f"{d}-{r}x{c}-k{k}" for d, r, c, k in KBEST])
def test_kbest_against_the_reference(sh, dtype, nr, nc, k):
    hi = 16 if nr == 8 else 1 << 20  # (8 x 8: ties between the ranks)
    B = 2 if nc < 200 else 1
    _, cost, count = check_kbest(sh, costs(B, nr, nc, 21, hi=hi), k, dtype=dtype, certify=nc in (65, 257))
    assert (count == k).all() and (np.diff(cost, axis=1) >= 0).all()


def test_kbest_is_deterministic(sh):
    Ct = torch.from_numpy(costs(4, 40, 44, 22, hi=8)).cuda()
    a = sh.kbest_batched(Ct, 12)
    b = sh.kbest_batched(Ct, 12)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", TORCH)
def test_k_one_is_the_cold_solve_bit_for_bit(sh, dtype):
    for nr, nc in ((5, 5), (64, 64), (60, 65), (257, 257)):
        Ct = torch.from_numpy(costs(3, nr, nc, 23)).to(TORCH[dtype]).cuda()
        cols, cost, count = sh.kbest_batched(Ct, 1)
        col, c1 = sh.solve_batched_large(Ct)
        assert torch.equal(cols[:, 0], col) and cost[:, 0].cpu().numpy().tobytes() == c1.cpu().numpy().tobytes()
        assert count.cpu().tolist() == [1, 1, 1]


def test_three_by_three_has_six_assignments(sh):
    C = costs(1, 3, 3, 24, hi=100)[0]
    cols, cost = sh.kbest_assignments(C, 10)
    assert cols.shape == (6, 3) and cols.dtype == np.int64 and cost.shape == (6,)
    assert same(cost, KF.brute_force(C))
    bc, bcost, count = sh.kbest_batched(torch.from_numpy(C).cuda()[None], 10)
    assert count.item() == 6 and bool((bc[0, 6:] == -1).all()) and bool((bcost[0, 6:] == INF).all())
    KF.check_assignments(C, bc[0].cpu().numpy(), bcost[0].cpu().numpy(), 6)


def test_an_infeasible_root_has_no_assignment(sh):
    C = costs(2, 4, 5, 25, hi=9)
    C[0, 2] = np.inf
    cols, cost, count = sh.kbest_batched(torch.from_numpy(C).cuda(), 4)
    assert count.cpu().tolist() == [0, 4]
    assert bool((cols[0] == -1).all()) and bool((cost[0] == INF).all())
    cols1, cost1 = sh.kbest_assignments(C[0], 4)
    assert cols1.shape == (0, 4) and cost1.shape == (0,)


def test_maximize_negates_the_problem(sh):
    Ch = costs(2, 6, 7, 26, hi=12)
    Ct = torch.from_numpy(Ch).cuda()
    cols, cost, count = sh.kbest_batched(Ct, 9, maximize=True)
    mcols, mcost, mcount = sh.kbest_batched(-Ct, 9)
    assert torch.equal(cols, mcols) and torch.equal(cost, -mcost) and torch.equal(count, mcount)
    for b in range(2):
        rcols, rcost, rcount, _, _ = KR.kbest(-Ch[b], 9)
        assert same(cols[b].cpu().numpy(), rcols) and same(cost[b].cpu().numpy(), -rcost) and count[b].item() == rcount
    # exhausted ranks read -inf
    c1, k1, n1 = sh.kbest_batched(Ct[:, :2, :2].contiguous(), 5, maximize=True)
    assert n1.cpu().tolist() == [2, 2] and bool((k1[:, 2:] == -INF).all()) and bool((c1[:, 2:] == -1).all())
    ci, ki = sh.kbest_assignments(Ch[0], 3, maximize=True)
    assert same(ci, cols[0, :3].cpu().numpy()) and same(ki, cost[0, :3].cpu().numpy())


def test_a_tall_batch_is_solved_as_its_transpose(sh):
    Ch = costs(2, 5, 3, 27, hi=10)
    cols, cost, count = sh.kbest_batched(torch.from_numpy(Ch).cuda(), 8)
    assert tuple(cols.shape) == (2, 8, 5)
    cols, cost, count = cols.cpu().numpy(), cost.cpu().numpy(), count.cpu().numpy()
    for b in range(2):
        rcols, rcost, rcount, _, _ = KR.kbest(Ch[b].T, 8)  # (row of the tall matrix for each of its columns)
        assert count[b] == rcount == 8 and cost[b].tobytes() == rcost.tobytes()
        for r in range(8):
            want = -np.ones(5, dtype=np.int64)
            want[rcols[r]] = np.arange(3)
            assert same(cols[b, r], want), (b, r)
    ci, ki = sh.kbest_assignments(Ch[0], 2)
    assert same(ci, cols[0, :2]) and same(ki, cost[0, :2])


def test_generic_floats_valid_ordered_and_within_the_rounding_bound(sh):
    B, nr, nc, k = 3, 40, 43, 6
    Ch = np.random.default_rng(28).random((B, nr, nc))
    for dtype in TORCH:
        Ct = torch.from_numpy(Ch).to(TORCH[dtype]).cuda()
        cols, cost, count = [x.cpu().numpy() for x in sh.kbest_batched(Ct, k)]
        Cw = Ct.double().cpu().numpy()
        assert (count == k).all() and (np.diff(cost, axis=1) >= 0).all()
        for b in range(B):
            assert len({tuple(c) for c in cols[b].tolist()}) == k
            for r in range(k):
                c = cols[b, r].astype(np.int64)
                assert ((c >= 0) & (c < nc)).all() and np.unique(c).size == nr
                chosen = Cw[b, np.arange(nr), c]
                assert abs(cost[b, r] - math.fsum(chosen)) <= (nr - 1) * 2.0 ** -53 * math.fsum(np.abs(chosen)), (b, r)
