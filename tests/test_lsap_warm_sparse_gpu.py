"""GPU tests of the warm start on sparse (CSR) costs: resolve_batched_sparse
and linear_sum_assignment_sparse_resolve (the lsap_warm_csr_ entries).

The contract is one sentence -- a sparse warm solve returns what the dense warm
solve returns for the densification, from the same shapes and the same previous
(col, v) -- so the yardstick is resolve_batched on padded_dense of the same
batch (existing code, not code under test): col and kept the same integers,
cost the same bits, u and v equal by value (np.array_equal with NaN == NaN: a
zero's sign is not compared, because a walk over stored entries meets them in
another order than the dense row walk and the minimum by value may keep either
zero).  Up to 257 columns the host reference (tests/lsap_warm_ref.py on the
densification) is compared as well.  Every instance of every case of
tests/lsap_warm_sparse_families.py is compared; test_lsap_warm_sparse_cpu.py
shows on the CPU that those cases hold every kind of instance.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_sparse_families as S  # noqa: E402
import lsap_warm_ref as W  # noqa: E402
import lsap_warm_sparse_families as WS  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_BUILD_ONLY = 4
SH_HALL_DEFICIENT = 4
HOST_REFERENCE_MAX_NC = 257


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    assert hasattr(santa_hip, "resolve_batched_sparse"), "santa_hip has no resolve_batched_sparse"
    assert hasattr(santa_hip, "linear_sum_assignment_sparse_resolve")
    assert santa_hip.SH_HALL_DEFICIENT == SH_HALL_DEFICIENT
    return santa_hip


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return np.array_equal(a, b, equal_nan=True)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def device_csr(b, dtype=torch.float64):
    return (torch.from_numpy(b.indptr).cuda(), torch.from_numpy(b.indices).cuda(),
            torch.from_numpy(b.data).to(dtype).cuda())


def shapes_of(b):
    return None if b.corners is None else np.asarray(b.corners, dtype=np.int32)


def both(sh, b, nr, nc, col0, v0, flags=0, shapes="own", **kw):
    """(sparse result, dense result) of one warm solve of batch b from (col0, v0)."""
    B = len(b.dense)
    shapes = shapes_of(b) if isinstance(shapes, str) else shapes
    crow, idx, val = device_csr(b)
    u0 = torch.zeros((B, nr), dtype=torch.float64, device="cuda")
    before = (col0.clone(), v0.clone(), crow.clone(), idx.clone(), val.clone())
    got = sh.resolve_batched_sparse(crow, idx, val, (B, nr, nc), col0, u0, v0, flags=flags, shapes=shapes, **kw)
    for x, y in zip((col0, v0, crow, idx, val), before):
        assert same(x, y), "an input was modified"
    D = torch.from_numpy(S.padded_dense(b, nr, nc)).cuda()
    want = sh.resolve_batched(D, col0, u0, v0, flags=flags, shapes=shapes, **kw)
    return got, want


def assert_contract(got, want):
    col, cost, u, v, kept = got
    dcol, dcost, du, dv, dkept = want
    assert col.dtype == torch.int32 and kept.dtype == torch.int32 and u.dtype == v.dtype == torch.float64
    assert torch.equal(col, dcol), "col"
    assert torch.equal(kept, dkept), "kept"
    assert same(u, du), "u"
    assert same(v, dv), "v"
    if dcost is None:
        assert cost is None
    else:
        assert cost.dtype == torch.float64 and same_bits(cost, dcost), "cost"


def garbage_col(rng, B, nr, nc):
    return torch.from_numpy(rng.integers(-5, nc + 5, size=(B, nr)).astype(np.int32)).cuda()


def garbage_v(rng, B, nc):
    v = rng.integers(-40, 9, size=(B, nc)).astype(np.float64)  # (positive values among them)
    bad = rng.random((B, nc))
    v[bad < 0.05] = np.nan
    v[(bad >= 0.05) & (bad < 0.10)] = np.inf
    v[(bad >= 0.10) & (bad < 0.15)] = -np.inf
    return torch.from_numpy(v).cuda()


# --------------------------------------------------------------------------- 1: the prologue alone
PROLOGUE_SHAPES = ((64, 64), (63, 65), (40, 129), (100, 257))
PROLOGUE_FAMILIES = ("band_5pct", "word_edges", "explicit_zero", "empty_row", "ragged")
STATES = ("cold", "garbage_col", "garbage_v", "garbage_both")


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("nr,nc", PROLOGUE_SHAPES, ids=[f"{r}x{c}" for r, c in PROLOGUE_SHAPES])
def test_prologue_alone_equals_the_reference_entry_by_entry(sh, nr, nc, state):
    for family in PROLOGUE_FAMILIES:
        w = WS.perturbed(family, nr, nc)
        b, B = w.batch, len(w.batch.dense)
        rng = np.random.default_rng([7, nr, nc, STATES.index(state)])
        col0 = garbage_col(rng, B, nr, nc) if state in ("garbage_col", "garbage_both") else \
            torch.from_numpy(w.col0).cuda()
        v0 = garbage_v(rng, B, nc) if state in ("garbage_v", "garbage_both") else torch.from_numpy(w.v0).cuda()
        got, want = both(sh, b, nr, nc, col0, v0, flags=SH_FLAG_BUILD_ONLY)
        assert_contract(got, want)
        col, cost, u, v, kept = (x.cpu().numpy() for x in got)
        assert not cost.any(), "SH_FLAG_BUILD_ONLY returns cost 0"
        c0, v0h = col0.cpu().numpy(), v0.cpu().numpy()
        for k, D in enumerate(b.dense):
            r, c = D.shape
            tag = (family, k)
            assert (col[k, r:] == -1).all() and not u[k, r:].any() and not v[k, c:].any(), tag
            if r == 0:
                assert kept[k] == 0, tag
                continue
            try:
                wc, _, wu, wv, wkept = W.prologue(D, c0[k, :r], v0h[k, :c])
            except ValueError:  # a row without an edge: -1, NaN in the live slots, kept 0
                wc, wu, wv, wkept = -np.ones(r), np.full(r, np.nan), np.full(c, np.nan), 0
            assert same(col[k, :r], wc), tag
            assert same(u[k, :r], wu), tag
            assert same(v[k, :c], wv), tag
            assert kept[k] == wkept, tag


# --------------------------------------------------------------------------- 2: the full warm solve
def rows_without_an_edge(D):
    return not np.isfinite(D).any(axis=1).all()


@pytest.mark.parametrize("family,nr,nc", WS.cases())
def test_sparse_warm_solve_is_the_dense_warm_solve_of_the_densification(sh, family, nr, nc):
    w, src = WS.perturbed(family, nr, nc), S.batch(family, nr, nc)
    b, B = w.batch, len(w.batch.dense)
    shapes = shapes_of(b)
    col0, v0 = torch.from_numpy(w.col0).cuda(), torch.from_numpy(w.v0).cuda()
    got, want = both(sh, b, nr, nc, col0, v0)
    assert_contract(got, want)
    col, cost, u, v, kept = got
    colh, costh, uh, vh, kepth = (x.cpu().numpy() for x in got)
    # certified on the CSR itself: optimal where there is an assignment, provably none where there is not
    crow, idx, val = device_csr(b)
    cflags = sh.check_duals_sparse(crow, idx, val, (B, nr, nc), col, u, v, shapes=shapes)[1].cpu().numpy()
    match, card, wit = sh.maximum_matching_sparse(crow, idx, val, shape=(B, nr, nc), shapes=shapes)
    hflags = sh.check_matching_sparse(crow, idx, val, (B, nr, nc), match, wit, shapes=shapes)[1].cpu().numpy()
    for k, D in enumerate(b.dense):
        r, c = D.shape
        tag = (family, nr, nc, k)
        assert (colh[k, r:] == -1).all() and not uh[k, r:].any() and not vh[k, c:].any(), tag
        if r == 0:
            assert (colh[k] == -1).all() and costh[k] == 0 and kepth[k] == 0 and not uh[k].any() and not vh[k].any()
            continue
        if (colh[k, :r] >= 0).any():
            assert (colh[k, :r] >= 0).all() and cflags[k] == 0, (tag, cflags[k])
            assert hflags[k] == 0, tag
        else:
            assert costh[k] == 0 and np.isnan(uh[k, :r]).all() and np.isnan(vh[k, :c]).all(), tag
            assert hflags[k] == SH_HALL_DEFICIENT, (tag, hflags[k])
            if rows_without_an_edge(D):
                assert kepth[k] == 0, tag
        if r == c and src.feasible[k] and not rows_without_an_edge(D):
            assert kepth[k] >= r - 4, (tag, kepth[k])  # (at most four rows were changed)
        if nc <= HOST_REFERENCE_MAX_NC:
            try:
                wc, wu, wv, wkept, searches = W.warm(D, w.col0[k, :r], w.v0[k, :c])
            except ValueError:
                assert (colh[k, :r] == -1).all(), tag
                continue
            assert searches == r - wkept
            assert same(colh[k, :r], wc) and same(uh[k, :r], wu) and same(vh[k, :c], wv), tag
            assert kepth[k] == wkept and costh[k] == D[np.arange(r), wc].sum(), tag


# --------------------------------------------------------------------------- 3: the fixed point
@pytest.mark.parametrize("family,nr,nc", WS.cases())
def test_a_cold_sparse_solution_is_a_fixed_point(sh, family, nr, nc):
    b = WS.perturbed(family, nr, nc).batch
    B = len(b.dense)
    shapes = shapes_of(b)
    crow, idx, val = device_csr(b)
    col0, cost0, u0, v0 = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), shapes=shapes, duals=True)
    col, cost, u, v, kept = sh.resolve_batched_sparse(crow, idx, val, (B, nr, nc), col0, u0, v0, shapes=shapes)
    assert torch.equal(col, col0) and same(u, u0) and same(v, v0) and same_bits(cost, cost0)
    for k, D in enumerate(b.dense):
        if D.shape[0] and int(col0[k, 0]) >= 0:
            assert int(kept[k]) == D.shape[0], (k, int(kept[k]))


# --------------------------------------------------------------------------- 4: small checks
@pytest.mark.parametrize("family,nr,nc", [("band_5pct", 63, 65), ("word_edges", 100, 513), ("band_40pct", 40, 2049)])
def test_float32_storage_gives_float64_storages_outputs(sh, family, nr, nc):
    w = WS.perturbed(family, nr, nc)
    b, B = w.batch, len(w.batch.dense)
    col0, v0 = torch.from_numpy(w.col0).cuda(), torch.from_numpy(w.v0).cuda()
    u0 = torch.zeros((B, nr), dtype=torch.float64, device="cuda")
    crow, idx, val = device_csr(b)
    for flags in (0, SH_FLAG_BUILD_ONLY):
        a = sh.resolve_batched_sparse(crow, idx, val, (B, nr, nc), col0, u0, v0, flags=flags)
        f = sh.resolve_batched_sparse(crow, idx, val.float(), (B, nr, nc), col0, u0, v0, flags=flags)
        assert torch.equal(a[0], f[0]) and same_bits(a[1], f[1]) and same(a[2], f[2]) and same(a[3], f[3])
        assert torch.equal(a[4], f[4])


def test_without_cost_other_col_dtypes_and_one_sparse_tensor(sh):
    family, nr, nc = "band_5pct", 100, 257
    w = WS.perturbed(family, nr, nc)
    b, B = w.batch, len(w.batch.dense)
    col0, v0 = torch.from_numpy(w.col0).cuda(), torch.from_numpy(w.v0).cuda()
    got, want = both(sh, b, nr, nc, col0, v0, with_cost=False)
    assert got[1] is None
    assert_contract(got, want)
    full = both(sh, b, nr, nc, col0, v0)[0]
    assert torch.equal(full[0], got[0]) and same(full[2], got[2]) and same(full[3], got[3])
    crow, idx, val = device_csr(b)
    u0 = torch.zeros((B, nr), dtype=torch.float64, device="cuda")
    A = torch.sparse_csr_tensor(crow, idx.long(), val, size=(B * nr, nc))
    other = sh.resolve_batched_sparse(A, None, None, (B, nr, nc), col0.long(), u0, v0)
    assert_contract(other, full)


@pytest.mark.parametrize("family,nr,nc", [("band_5pct", 64, 64), ("explicit_zero", 100, 257), ("bidiagonal", 63, 65)])
def test_maximize_is_the_solve_of_the_negated_values(sh, family, nr, nc):
    w = WS.perturbed(family, nr, nc)
    b, B = w.batch, len(w.batch.dense)
    col0, v0 = torch.from_numpy(w.col0).cuda(), torch.from_numpy(w.v0).cuda()
    u0 = torch.zeros((B, nr), dtype=torch.float64, device="cuda")
    crow, idx, val = device_csr(b)
    col, cost, u, v, kept = sh.resolve_batched_sparse(crow, idx, val, (B, nr, nc), col0, u0, v0)
    mcol, mcost, mu, mv, mkept = sh.resolve_batched_sparse(crow, idx, -val, (B, nr, nc), col0, -u0, -v0,
                                                            maximize=True)
    assert torch.equal(col, mcol) and torch.equal(kept, mkept)
    assert same(cost, -mcost) and same(u, -mu) and same(v, -mv)


def test_ragged_with_its_empty_shape_and_an_invalid_one(sh):
    family, nr, nc = "ragged", 40, 129
    w = WS.perturbed(family, nr, nc)
    b = w.batch
    assert (0, 0) in [tuple(c) for c in b.corners], "the ragged family holds its empty shape"
    col0, v0 = torch.from_numpy(w.col0).cuda(), torch.from_numpy(w.v0).cuda()
    got, want = both(sh, b, nr, nc, col0, v0)
    assert_contract(got, want)
    # an invalid shape reaches the kernels only past the front end's checks: through the C entry
    import ctypes
    from santa_hip import _lib
    from santa_hip.context import current_stream_handle
    B = len(b.dense)
    bad = shapes_of(b).copy()
    bad[0] = (5, 3)        # nr_b > nc_b
    bad[1] = (nr + 1, nc)  # more rows than the padded matrix has
    sdev = torch.from_numpy(bad).cuda()
    crow, idx, val = device_csr(b)
    col, v = col0.clone(), v0.clone()
    u = torch.full((B, nr), 7.0, dtype=torch.float64, device="cuda")
    cost = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    kept = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    nbytes = int(L.lsap_csr_work_bytes(nr, nc, B))
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lsap_warm_csr_f64(p(crow), p(idx), p(val), nr, nc, B, p(sdev), p(col), p(cost), p(u), p(v), p(kept),
                             p(work), nbytes, 0, current_stream_handle(torch.device("cuda")))
    assert rc == _lib.SH_OK
    torch.cuda.synchronize()
    for k in (0, 1):
        assert bool((col[k] == -1).all()) and float(cost[k]) == 0 and int(kept[k]) == 0
        assert not u[k].any() and not v[k].any()
    assert torch.equal(col[2:], got[0][2:]) and same_bits(cost[2:], got[1][2:]) and torch.equal(kept[2:], got[4][2:])
    assert same(u[2:], got[2][2:]) and same(v[2:], got[3][2:])


# --------------------------------------------------------------------------- 5: one matrix
@pytest.mark.parametrize("nr,nc", [(40, 40), (30, 45), (45, 30)])
@pytest.mark.parametrize("maximize", (False, True))
def test_linear_sum_assignment_sparse_resolve_reaches_scipys_optimum(sh, nr, nc, maximize):
    scipy_opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng([3, nr, nc])
    P = rng.random((nr, nc)) < 0.3
    P[np.arange(min(nr, nc)), np.arange(min(nr, nc))] = True
    V = rng.integers(0, 64, size=(nr, nc)).astype(np.float64)
    A = S.csr_of(P, V) + ((nr, nc),)
    rows, cols, u, v = sh.linear_sum_assignment_sparse(A, maximize=maximize, duals=True)
    col_ind = np.full(nr, -1, dtype=np.int64)
    col_ind[rows] = cols
    # a nearby matrix: two chosen entries leave the pattern, one missing entry arrives as the best there is
    P2, V2 = P.copy(), V.copy()
    P2[rows[3], cols[3]] = P2[rows[7], cols[7]] = False
    gap = np.argwhere(~P)[0]
    P2[gap[0], gap[1]] = True
    V2[gap[0], gap[1]] = 100.0 if maximize else -5.0
    A2 = S.csr_of(P2, V2) + ((nr, nc),)
    r2, c2, u2, v2 = sh.linear_sum_assignment_sparse_resolve(A2, col_ind, u, v, maximize=maximize)
    D2 = np.where(P2, V2, -np.inf if maximize else np.inf)
    wr, wc = scipy_opt.linear_sum_assignment(D2, maximize=maximize)
    assert r2.dtype == np.int64 and c2.dtype == np.int64 and u2.shape == (nr,) and v2.shape == (nc,)
    assert np.array_equal(r2, wr) and np.unique(c2).size == c2.size
    assert D2[r2, c2].sum() == D2[wr, wc].sum()
    # the duals prove it: feasible everywhere, tight on the chosen pairs (integers: exact)
    red = D2 - u2[:, None] - v2[None, :]
    assert (red <= 0).all() if maximize else (red >= 0).all()
    assert not red[r2, c2].any()


def test_linear_sum_assignment_sparse_resolve_raises_on_infeasible_input(sh):
    P = np.eye(6, dtype=bool)
    P[2] = P[4] = False
    P[[2, 4], 5] = True  # two rows whose only column is shared
    A = S.csr_of(P, np.ones((6, 6))) + ((6, 6),)
    with pytest.raises(ValueError, match="infeasible"):
        sh.linear_sum_assignment_sparse_resolve(A, np.arange(6), np.zeros(6), np.zeros(6))
    with pytest.raises(ValueError, match="infeasible"):
        sh.linear_sum_assignment_sparse_resolve((A[0], A[1], A[2], (6, 6)), np.full(6, -1), np.zeros(6), np.zeros(6),
                                                maximize=True)
