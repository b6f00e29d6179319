"""GPU tests of the free-rows warm start (resolve_batched_free_rows,
linear_sum_assignment_resolve(free_rows=True), the lsap_warm_fr_ entries;
DESIGN.md §22).

The mode is defined as the existing warm start of the written-out padded
matrix, so that is what every result is compared with, entry by entry:
resolve_batched on vstack(C, zeros) from the start state's pairs
(tests/free_rows_ref.start_state gives the columns of the virtual rows).

  col[:nr], kept, kept_free   equal
  cost                        equal bits (the zero rows add 0)
  float costs: u, v           equal bits; theta == max v
  integer costs: u, v         equal after the exact shift by theta = max v
                              of the padded problem, and theta equal

and every integer result is certified with check_duals_large on the unpadded
matrix.  Costs are integer-valued (also in the float dtypes) except in the one
test of fractional float64 costs.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import free_rows_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_BUILD_ONLY = 4
# every seam of launch_warm's table
SIZES = (2, 5, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
NARROW = {"int32": torch.int32, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
TORCH = dict(NARROW, int64=torch.int64, float64=torch.float64)


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    assert hasattr(santa_hip, "resolve_batched_free_rows"), "santa_hip has no resolve_batched_free_rows"
    return santa_hip


def bits(t):
    """A tensor's values as integers: equal bits <=> equal entries (NaN and the sign of a zero included)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64).numpy() if t.dtype == torch.float64 else t.numpy()


def host(Ct):
    return (Ct.double() if Ct.is_floating_point() else Ct.long()).cpu().numpy()


def costs(dtype, B, nr, nc, seed, hi=1 << 20):
    C = np.random.default_rng([seed, nr, nc]).integers(0, hi, size=(B, nr, nc), dtype=np.int64)
    return torch.from_numpy(C).to(TORCH[dtype]).cuda()


def cold_state(sh, Ct, shapes=None):
    col, _, u, v = sh.solve_batched_large(Ct, duals=True, shapes=shapes)
    return col, v


def redraw(Ct, rng, k, hi=1 << 20):
    """k rows of every instance drawn again."""
    D = Ct.clone()
    B, nr, nc = D.shape
    for b in range(B):
        rows = rng.choice(nr, size=min(k, nr), replace=False)
        D[b, torch.from_numpy(rows).cuda()] = torch.from_numpy(
            rng.integers(0, hi, size=(len(rows), nc))).to(D.dtype).cuda()
    return D


def garbage(rng, B, nr, nc, ddt):
    """Columns out of range and duplicated; duals positive, far below the window, and for floats NaN and -inf."""
    col = torch.from_numpy(rng.integers(-5, nc + 5, size=(B, nr))).cuda()
    v = rng.integers(-(1 << 19), 1 << 17, size=(B, nc)).astype(np.float64 if ddt == torch.float64 else np.int64)
    if ddt == torch.float64:
        v[rng.random((B, nc)) < 0.1] = np.nan
        v[rng.random((B, nc)) < 0.1] = -np.inf
    else:
        v[rng.random((B, nc)) < 0.1] = -(1 << 60)
    return col, torch.from_numpy(v).cuda()


def check(sh, D, col0, v0, shapes=None, certify=True):
    """One call against the warm start of the written-out padded matrices -> its outputs."""
    ddt = torch.float64 if D.is_floating_point() else torch.int64
    B, NR, NC = D.shape
    before = (col0.clone(), v0.clone())
    zu = torch.zeros((B, NR), dtype=ddt, device="cuda")
    out = sh.resolve_batched_free_rows(D, col0, zu, v0, shapes=shapes)
    col, cost, u, v, kept, kept_free, theta = out
    assert torch.equal(col0, before[0]) and np.array_equal(bits(v0), bits(before[1])), "inputs were modified"
    assert col.dtype == kept.dtype == kept_free.dtype == torch.int32
    assert cost.dtype == u.dtype == v.dtype == theta.dtype == ddt
    again = sh.resolve_batched_free_rows(D, col0, zu, v0, shapes=shapes)
    for a, b in zip(out, again):
        assert np.array_equal(bits(a), bits(b)), "two runs differ"
    Dh, colh, vh = host(D), col0.cpu().numpy(), v0.cpu().numpy()
    sizes = [(NR, NC)] * B if shapes is None else [tuple(s) for s in np.asarray(shapes).tolist()]
    ext = np.full((B, NC), -1, dtype=np.int64)   # the padded problems' previous assignments
    want_kept = np.zeros((B, 2), dtype=np.int64)
    dead = []  # instances the padded call answers differently by construction
    for b, (nr, nc) in enumerate(sizes):
        if nr == 0:
            dead.append(b)
            continue
        try:
            _, c4r, _, _, _, k, kf = FR.start_state(Dh[b, :nr, :nc], colh[b, :nr], vh[b, :nc])
            ext[b, :nc] = c4r
            want_kept[b] = (k, kf)
        except ValueError:   # a row of +inf: the prologue itself sees it
            pass
    P = torch.zeros((B, NC, NC), dtype=D.dtype, device="cuda")   # the written-out padded matrices
    for b, (nr, nc) in enumerate(sizes):
        P[b, :nr] = D[b, :nr]
    pshapes = None if shapes is None else [[nc, nc] for _, nc in sizes]
    pc, pcost, pu, pv, pkept = sh.resolve_batched(P, torch.from_numpy(ext).cuda(),
                                                  torch.zeros((B, NC), dtype=ddt, device="cuda"), v0, shapes=pshapes)
    for b, (nr, nc) in enumerate(sizes):
        if b in dead:
            assert (col[b] == -1).all() and not cost[b] and not u[b].any() and not v[b].any()
            assert kept[b] == 0 and kept_free[b] == 0 and theta[b] == 0
            continue
        assert torch.equal(col[b, :nr], pc[b, :nr]), b
        assert (col[b, nr:] == -1).all(), b
        assert np.array_equal(bits(cost[b]), bits(pcost[b])), b
        infeasible = bool((pc[b, :nc] < 0).any())
        if infeasible:
            assert (col[b] == -1).all() and bool(torch.isnan(theta[b])) and bool(torch.isnan(u[b, :nr]).all())
            assert bool(torch.isnan(v[b, :nc]).all()) and cost[b] == 0
            continue
        assert [int(kept[b]), int(kept_free[b])] == want_kept[b].tolist(), b
        assert int(kept[b]) + int(kept_free[b]) == int(pkept[b]), b
        th = pv[b, :nc].max()
        shift = th if (ddt == torch.int64 and nr < nc) else torch.zeros((), dtype=ddt, device="cuda")
        assert theta[b] == th, b
        if ddt == torch.float64:   # no shift: the padded problem's duals bit for bit
            assert np.array_equal(bits(u[b, :nr]), bits(pu[b, :nr])), b
            assert np.array_equal(bits(v[b, :nc]), bits(pv[b, :nc])), b
        else:
            assert torch.equal(u[b, :nr], pu[b, :nr] + shift) and torch.equal(v[b, :nc], pv[b, :nc] - shift), b
        assert not u[b, nr:].any() and not v[b, nc:].any(), b
    if certify and ddt == torch.int64:
        fl = sh.check_duals_large(D, col, u, v, shapes=shapes)[3]
        assert fl.cpu().tolist() == [0] * B
    return out


def rows_of(nc):
    return sorted({nr for nr in (nc - 1, nc - 7, 1, 3, nc) if 1 <= nr <= nc})


SWEEP = [(dt, nr, nc) for nc in SIZES for nr in rows_of(nc) for dt in ("int64", "float64")]


@pytest.mark.parametrize("dtype,nr,nc", SWEEP, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in SWEEP])
def test_every_seam_from_solved_redrawn_garbage_and_empty_states(sh, dtype, nr, nc):
    big = nc > 1025
    B = 1 if big else 3
    Ct = costs(dtype, B, nr, nc, 2)
    col, v = cold_state(sh, Ct)
    rng = np.random.default_rng([21, nr, nc])
    out = check(sh, Ct, col, v)                                   # the solved state, unchanged
    assert out[4].tolist() == [nr] * B and out[5].tolist() == [nc - nr] * B and torch.equal(out[0], col)
    out = check(sh, redraw(Ct, rng, 1), col, v)                   # one redrawn row
    assert int(out[4].min()) >= nr - 1 and out[5].tolist() == [nc - nr] * B
    if big:   # (above 1025 columns: one instance and at most two redrawn rows)
        out = check(sh, redraw(Ct, rng, 2), col, v)
        assert int(out[4].min()) >= nr - 2 and out[5].tolist() == [nc - nr] * B
        return
    check(sh, redraw(Ct, rng, 2), *garbage(rng, B, nr, nc, v.dtype))
    out = check(sh, Ct, torch.full_like(col, -1), torch.zeros_like(v))   # the empty state
    assert not out[4].any() and out[5].tolist() == [nc - nr] * B


NARROW_CASES = [(dt, nr, nc) for dt in NARROW for nc in (65, 257, 1025) for nr in (nc, nc - 7, 3)]


@pytest.mark.parametrize("dtype,nr,nc", NARROW_CASES, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in NARROW_CASES])
def test_narrow_dtypes_on_integer_valued_costs(sh, dtype, nr, nc):
    Ct = costs(dtype, 3, nr, nc, 3, 64)   # [0, 64): exact in every dtype and in every sum
    col, v = cold_state(sh, Ct)
    rng = np.random.default_rng([23, nr, nc])
    check(sh, redraw(Ct, rng, 1, 64), col, v)
    check(sh, redraw(Ct, rng, 2, 64), *garbage(rng, 3, nr, nc, v.dtype))


def test_fractional_float64_costs(sh):
    rng = np.random.default_rng(24)
    for nr, nc in ((58, 65), (250, 257), (3, 64)):
        Ct = torch.from_numpy(rng.random((3, nr, nc)) * 100.0).cuda()
        col, v = cold_state(sh, Ct)
        D = Ct.clone()
        D[:, nr // 2] = torch.from_numpy(rng.random((3, nc)) * 100.0).cuda()
        c1, cost1, u1, v1, k1, kf1, th1 = check(sh, D, col, v)
        # its own result fed back: the duals are a state of the padded problem, nothing is recomputed wrongly
        c2, cost2, *_ = check(sh, D, c1, v1)
        assert torch.equal(c1, c2) and torch.equal(cost1, cost2)


def test_ragged_batch_with_a_padded_and_an_empty_instance(sh):
    for dtype in ("int64", "float64"):
        NR, NC = 70, 80
        shapes = [[70, 80], [33, 64], [1, 1], [0, 0], [64, 65], [5, 80], [40, 40]]
        B = len(shapes)
        Ct = costs(dtype, B, NR, NC, 5)
        col, v = cold_state(sh, Ct, shapes)
        rng = np.random.default_rng(25)
        check(sh, redraw(Ct, rng, 1), col, v, shapes=shapes)
        check(sh, redraw(Ct, rng, 1), *garbage(rng, B, NR, NC, v.dtype), shapes=shapes)


def test_build_only_returns_the_start_state(sh):
    for dtype in ("int64", "float64"):
        for nr, nc in ((58, 65), (250, 257), (3, 1025), (65, 65)):
            B = 2
            Ct = costs(dtype, B, nr, nc, 6)
            col, v = cold_state(sh, Ct)
            rng = np.random.default_rng([26, nr, nc])
            D = redraw(Ct, rng, 2)
            for col0, v0 in ((col, v), garbage(rng, B, nr, nc, v.dtype)):
                gc, gcost, gu, gv, gk, gkf, gth = sh.resolve_batched_free_rows(
                    D, col0, torch.zeros_like(v[:, :nr]), v0, flags=SH_FLAG_BUILD_ONLY)
                Dh = host(D)
                for b in range(B):
                    _, c4r, _, su, sv, k, kf = FR.start_state(Dh[b], col0[b].cpu().numpy(), v0[b].cpu().numpy())
                    assert np.array_equal(gc[b].cpu().numpy(), c4r[:nr])
                    assert np.array_equal(gu[b].cpu().numpy(), su[:nr]) and np.array_equal(gv[b].cpu().numpy(), sv)
                    assert (int(gk[b]), int(gkf[b])) == (k, kf)
                    assert gth[b].item() == sv.dtype.type(0) - FR.neg_theta(sv)
                assert not gcost.any()


def test_float_infeasibility(sh):
    C = np.random.default_rng(27).integers(0, 50, size=(4, 6, 9)).astype(np.float64)
    C[1, 2] = np.inf        # a row of +inf: the prologue sees it
    C[2, :2, 1:] = np.inf   # two rows that both need column 0: the continuation sees it
    Ct = torch.from_numpy(C).cuda()
    col0 = torch.arange(6, dtype=torch.int32).repeat(4, 1).cuda()
    col, cost, u, v, kept, kept_free, theta = check(sh, Ct, col0, torch.zeros((4, 9), dtype=torch.float64).cuda())
    assert (col[[1, 2]] == -1).all() and (col[[0, 3]] >= 0).all()
    assert torch.isnan(theta[[1, 2]]).all() and torch.isnan(u[[1, 2]]).all() and torch.isnan(v[[1, 2]]).all()
    assert kept[1] == 0 and kept_free[1] == 0 and not cost[[1, 2]].any()


@pytest.mark.parametrize("dtype", ("int64", "float64"))
@pytest.mark.parametrize("nr,nc", ((57, 64), (250, 256), (16, 128)))
def test_k_redrawn_rows_cost_at_most_k_searches(sh, dtype, nr, nc):
    B = 4
    Ct = costs(dtype, B, nr, nc, 7, 1 << 16)
    col, v = cold_state(sh, Ct)
    rng = np.random.default_rng([28, nr, nc])
    for k in (1, 3):
        D = redraw(Ct, rng, k, 1 << 16)
        out = sh.resolve_batched_free_rows(D, col, torch.zeros_like(v[:, :nr]), v)
        assert int(out[4].min()) >= nr - k and out[5].tolist() == [nc - nr] * B   # searches <= k
        want = sh.solve_batched_large(D)[1]
        assert np.array_equal(bits(out[1]), bits(want))   # (integer-valued: every sum is exact)


def test_square_instances_get_what_resolve_batched_returns(sh):
    for dtype in ("int64", "float64", "float32"):
        for n in (5, 64, 65, 257):
            Ct = costs(dtype, 3, n, n, 8, 64 if dtype == "float32" else 1 << 20)
            col, v = cold_state(sh, Ct)
            D = redraw(Ct, np.random.default_rng([29, n]), 2, 64)
            zu = torch.zeros_like(v)
            want = sh.resolve_batched(D, col, zu, v)
            got = sh.resolve_batched_free_rows(D, col, zu, v)
            for a, b in zip(got[:5], want):
                assert np.array_equal(bits(a), bits(b))
            assert not got[5].any() and torch.equal(got[6], got[3].max(dim=1).values)


def test_tall_batch_is_solved_as_its_transpose(sh):
    for dtype in ("int64", "float64"):
        B, nr, nc = 3, 40, 33   # tall: the wide problem is 33 x 40
        Ct = costs(dtype, B, nr, nc, 9)
        colT, _, uT, vT = sh.solve_batched_large(Ct.transpose(1, 2).contiguous(), duals=True)
        col, _, u, v = sh.solve_batched_large(Ct, duals=True)
        D = redraw(Ct.transpose(1, 2).contiguous(), np.random.default_rng(30), 1).transpose(1, 2).contiguous()
        got = sh.resolve_batched_free_rows(D, col, u, v)
        Dw = D.transpose(1, 2).contiguous()
        want = check(sh, Dw, colT, vT)
        assert np.array_equal(bits(got[1]), bits(want[1]))
        # the tall rows' duals are the wide problem's columns'
        assert np.array_equal(bits(got[2]), bits(want[3])) and np.array_equal(bits(got[3]), bits(want[2]))
        inv = torch.full((B, nr), -1, dtype=torch.int32, device="cuda")
        for b in range(B):
            inv[b, want[0][b].long()] = torch.arange(nc, dtype=torch.int32, device="cuda")
        assert torch.equal(got[0], inv)
        for a, b in zip(got[4:], want[4:]):
            assert np.array_equal(bits(a), bits(b))


def test_maximize_is_the_negated_problem(sh):
    for dtype in ("int64", "float64"):
        B, nr, nc = 3, 58, 65
        Ct = costs(dtype, B, nr, nc, 10)
        col, _, u, v = sh.solve_batched_large(Ct, duals=True, maximize=True)
        D = redraw(Ct, np.random.default_rng(31), 1)
        got = sh.resolve_batched_free_rows(D, col, u, v, maximize=True)
        want = check(sh, -D, col, -v)
        assert torch.equal(got[0], want[0]) and torch.equal(got[4], want[4]) and torch.equal(got[5], want[5])
        for i in (1, 2, 3, 6):   # cost, u, v, theta: the other sign
            assert np.array_equal(bits(got[i]), bits(-want[i])), i


def test_single_matrix_front_end(sh):
    rng = np.random.default_rng(32)
    for shape in ((30, 37), (37, 30), (12, 12)):
        C = rng.integers(0, 1000, size=shape)
        for M in (C, C + 0.5):
            r, c, u, v = sh.linear_sum_assignment_large(M, duals=True)
            col0 = np.full(shape[0], -1, dtype=np.int64)
            col0[r] = c
            D = M.copy()
            D[3] = rng.integers(0, 1000, size=shape[1]) + (M[0, 0] - C[0, 0])
            for maximize in (False, True):
                if maximize:
                    r, c, u, v = sh.linear_sum_assignment_large(M, maximize=True, duals=True)
                    col0[:] = -1
                    col0[r] = c
                fr, fc, fu, fv = sh.linear_sum_assignment_resolve(D, col0, u, v, maximize=maximize, free_rows=True)
                wr, wc = sh.linear_sum_assignment_large(D, maximize=maximize)
                assert D[fr, fc].sum() == D[wr, wc].sum() and len(set(fc.tolist())) == min(shape)
                slack = D - fu[:, None] - fv[None, :]
                assert (slack <= 0).all() if maximize else (slack >= 0).all()
                assert (slack[fr, fc] == 0).all()


# --------------------------------------------------------------------------- Murty's partition with free rows
import kbest_families as KF  # noqa: E402
import kbest_ref as KR  # noqa: E402

INF = float("inf")


def words(F, NC):
    """A bool mask over the columns as the int64 words of the entries' bitmap."""
    b = np.zeros(((NC + 63) // 64) * 64, dtype=bool)
    b[:len(F)] = F
    return np.packbits(b, bitorder="little").view(np.int64)


CHILDREN = [(dt, nc) for nc in (5, 64, 65, 256, 257, 513, 1024) for dt in ("float64", "float32")]


@pytest.mark.parametrize("dtype,nc", CHILDREN, ids=[f"{d}-{nc}" for d, nc in CHILDREN])
def test_children_against_resolve_batched_on_the_written_out_masked_padded_matrix(sh, dtype, nc):
    nr = nc - 3
    hi = 1 << 20 if dtype == "float64" else 1 << 10   # (integer-valued, exact in float32 and in every sum)
    Ch = np.random.default_rng([40, nc]).integers(0, hi, size=(1, nr, nc)).astype(np.float64)
    Ct = torch.from_numpy(Ch).to(TORCH[dtype]).cuda()
    rcol, _, _, rv = sh.solve_batched_large(Ct, duals=True)
    pcol, pv = rcol[0].cpu().numpy().astype(np.int64), rv[0].cpu().numpy()
    one = np.zeros(nc, dtype=bool)
    one[(pcol[nr // 2] + 1) % nc] = True
    masks = [np.zeros(nc, dtype=bool), one]
    if nc > 64:
        two = np.zeros(nc, dtype=bool)
        two[[63, 64]] = True
        masks.append(two)
    cases = [(p, F) for p in (0, nr // 2, nr - 1) for F in masks]
    B = len(cases)
    args = (rcol.repeat(B, 1), rv.repeat(B, 1), torch.tensor([p for p, _ in cases], dtype=torch.int32).cuda(),
            torch.from_numpy(np.stack([words(F, nc) for _, F in cases])).cuda())
    before = [a.clone() for a in args]
    out = sh.murty_children_batched(Ct.repeat(B, 1, 1), *args, free_rows=True)
    for a, b in zip(args, before):
        assert np.array_equal(bits(a), bits(b)), "inputs were modified"
    col, cost, u, v, kept = out
    assert tuple(col.shape) == (B, nr, nr) and tuple(v.shape) == (B, nr, nc) and tuple(kept.shape) == (B, nr)
    # the oracle: one padded matrix per child looked at, all in one resolve_batched call
    look, P, ext = [], [], []
    for q, (p, F) in enumerate(cases):
        assert (col[q, :p] == -1).all() and bool(torch.isinf(cost[q, :p]).all()) and not kept[q, :p].any()
        for t in sorted({p, (p + nr) // 2, nr - 1}):
            Ft = KR.forbidden_t(pcol, p, F, t)
            M = KR.masked(Ch[0], pcol, t, Ft)
            virtual = np.zeros(nc)
            virtual[pcol[:t]] = np.inf
            Pm, c4r, _, _, _, k, kf = FR.start_state(M, pcol, pv, virtual)
            look.append((q, t, k, kf))
            P.append(Pm)
            ext.append(c4r)
    n = len(look)
    pc, pcost, pu, pvv, pkept = sh.resolve_batched(
        torch.from_numpy(np.stack(P)).cuda(), torch.from_numpy(np.stack(ext)).cuda(),
        torch.zeros((n, nc), dtype=torch.float64, device="cuda"), rv.repeat(n, 1))
    for x, (q, t, k, kf) in enumerate(look):
        assert bool((pc[x] >= 0).all()), (q, t)   # (these children exist: three spare columns)
        assert torch.equal(col[q, t], pc[x, :nr]), (q, t)
        assert np.array_equal(bits(cost[q, t]), bits(pcost[x])), (q, t)
        assert np.array_equal(bits(u[q, t]), bits(pu[x, :nr])) and np.array_equal(bits(v[q, t]), bits(pvv[x])), (q, t)
        assert int(kept[q, t]) == k == nr - 1 and k + kf == int(pkept[x]) and kf == nc - nr, (q, t)


def check_kbest(sh, Ch, k, dtype="float64", shapes=None):
    """kbest_batched(free_rows=True) against the free-rows reference, entry by entry -> the host results."""
    B, NR, NC = Ch.shape
    Ct = torch.from_numpy(Ch).to(TORCH[dtype]).cuda()
    before = Ct.clone()
    cols, cost, count = sh.kbest_batched(Ct, k, shapes=shapes, free_rows=True)
    again = sh.kbest_batched(Ct, k, shapes=shapes, free_rows=True)
    assert np.array_equal(bits(Ct), bits(before)), "inputs were modified"
    for a, b in zip((cols, cost, count), again):
        assert np.array_equal(bits(a), bits(b)), "two runs differ"
    assert tuple(cols.shape) == (B, k, NR) and tuple(cost.shape) == (B, k) and tuple(count.shape) == (B,)
    cols, cost, count = cols.cpu().numpy(), cost.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        nr, nc = (NR, NC) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        if nr == 0:
            assert count[b] == 0 and (cols[b] == -1).all() and (cost[b] == INF).all(), b
            continue
        Cb = Ct[b, :nr, :nc].double().cpu().numpy()
        rcols, rcost, rcount, searches, _ = FR.kbest(Cb, k)
        assert count[b] == rcount, b
        assert np.array_equal(cols[b, :, :nr], rcols) and (cols[b, :, nr:] == -1).all(), b
        assert cost[b].tobytes() == rcost.tobytes(), b
        KF.check_assignments(Cb, cols[b, :, :nr], cost[b], int(count[b]))
    return cols, cost, count


def test_kbest_small_family_batched_and_ragged_in_one_call(sh):
    fam = KF.small_family()
    NR, NC = max(C.shape[0] for C in fam), max(C.shape[1] for C in fam)
    Ch = np.full((len(fam), NR, NC), 3.0)   # (the padding is never read)
    for b, C in enumerate(fam):
        Ch[b, :C.shape[0], :C.shape[1]] = C
    shapes = np.array([C.shape for C in fam])
    _, cost, count = check_kbest(sh, Ch, KF.K_SMALL, shapes=shapes)
    assert (count == 0).any() and ((count > 0) & (count < KF.K_SMALL)).any() and (count == KF.K_SMALL).any()
    for b, C in enumerate(fam):   # ... which is brute force's sequence
        want = KF.brute_force(C)
        assert np.array_equal(cost[b, :count[b]], want[:count[b]]) and count[b] == min(KF.K_SMALL, want.size)


KBEST = [("float64", 60, 67, 3), ("float32", 60, 67, 3), ("float64", 250, 256, 2), ("float32", 250, 256, 2),
         ("float64", 65, 65, 3)]


@pytest.mark.parametrize("dtype,nr,nc,k", KBEST, ids=[f"{d}-{r}x{c}-k{k}" for d, r, c, k in KBEST])
def test_kbest_against_the_reference_and_the_default_mode_s_costs(sh, dtype, nr, nc, k):
    B = 2 if nc < 200 else 1
    Ch = np.random.default_rng([41, nr, nc]).integers(0, 1 << 20, size=(B, nr, nc)).astype(np.float64)
    _, cost, count = check_kbest(sh, Ch, k, dtype=dtype)
    assert (count == k).all() and (np.diff(cost, axis=1) >= 0).all()
    # integer-valued costs: every sum is exact, so the default mode finds the same cost sequence, bit for bit
    Ct = torch.from_numpy(Ch).to(TORCH[dtype]).cuda()
    assert cost.tobytes() == sh.kbest_batched(Ct, k)[1].cpu().numpy().tobytes()


def test_kbest_tall_maximize_and_the_single_matrix_front_end(sh):
    rng = np.random.default_rng(42)
    Ch = rng.integers(0, 1000, size=(2, 12, 9)).astype(np.float64)   # tall
    Ct = torch.from_numpy(Ch).cuda()
    for maximize in (False, True):
        cols, cost, count = sh.kbest_batched(Ct, 6, maximize=maximize, free_rows=True)
        want = sh.kbest_batched(Ct, 6, maximize=maximize)
        assert np.array_equal(bits(cost), bits(want[1])) and torch.equal(count, want[2])
        for b in range(2):
            for r in range(6):
                c = cols[b, r].cpu().numpy()
                rows = np.flatnonzero(c >= 0)
                assert rows.size == 9 and len(set(c[rows].tolist())) == 9
                assert Ch[b, rows, c[rows]].sum() == cost[b, r].item()
        ac, acost = sh.kbest_assignments(Ch[0], 6, maximize=maximize, free_rows=True)
        assert np.array_equal(acost, cost[0].cpu().numpy()) and np.array_equal(ac, cols[0].cpu().numpy())
