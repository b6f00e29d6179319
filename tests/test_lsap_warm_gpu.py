"""GPU tests of the warm start (resolve_batched, linear_sum_assignment_resolve,
the lsap_warm_ entries) against tests/lsap_warm_ref.py.

The start state of a case is the GPU's own cold solve_batched_large(duals=True)
of the unperturbed costs, certified with check_duals_large (flags == 0); then
at most three rows are perturbed.  The warm result -- col, u, v, cost, kept --
is compared with replay_from(prologue(..)) entry by entry (np.array_equal: by
value, so a zero's sign is not compared; everything else is bit for bit, and
NaN matches NaN) and certified again.  Costs are integer-valued (also in the
float dtypes), so every sum is exact and equality needs no tolerance; one test
runs fractional float64 costs against the reference alone.

Host time: a wide instance (nr < nc) with costs from a wide range loses almost
every pair to the raise cascade, so its reference is a full replay; above 2049
columns the wide cases draw their costs from [0, 512), where ties leave most
column duals at 0, to keep the replay to a few seconds.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_duals_ref as R  # noqa: E402
import lsap_families as F  # noqa: E402
import lsap_warm_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_EXACT_ARGMIN = 2
SH_FLAG_BUILD_ONLY = 4
SIZES = (64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096)
NARROW = {"int32": torch.int32, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
TORCH = dict(NARROW, int64=torch.int64, float64=torch.float64)


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("resolve_batched", "linear_sum_assignment_resolve"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def is_float(dtype):
    return dtype.startswith("float") or dtype == "bfloat16"


def host(Ct):
    """The costs as the reference's int64 or float64 numpy array (exact)."""
    return (Ct.double() if Ct.is_floating_point() else Ct.long()).cpu().numpy()


def costs(dtype, B, nr, nc, seed, hi=1 << 20):
    C = np.random.default_rng([seed, nr, nc]).integers(0, hi, size=(B, nr, nc), dtype=np.int64)
    return torch.from_numpy(C).to(TORCH[dtype]).cuda()


def cold_state(sh, Ct):
    col, cost, u, v = sh.solve_batched_large(Ct, duals=True)
    fl = sh.check_duals_large(Ct, col, u, v)[3]
    assert fl.cpu().tolist() == [0] * Ct.shape[0]
    return col, cost, u, v


def perturb(Ct, col, rng, rows=3):
    """Up to `rows` changed entries per instance, in distinct rows: a matched
    entry made dearer, an unmatched one made the row's cheapest, a matched one
    made cheaper.  Values stay integers inside the dtype's exact range."""
    D = Ct.clone()
    B, nr, nc = D.shape
    colh = col.cpu().numpy()
    for b in range(B):
        pick = rng.choice(nr, size=min(rows, nr), replace=False)
        for t, i in enumerate(pick):
            j = int(colh[b, i])
            if t == 0:
                D[b, i, j] = D[b, i, j] + 37
            elif t == 1:
                D[b, i, (j + 1 + int(rng.integers(0, nc - 1))) % nc] = 0
            else:
                D[b, i, j] = D[b, i, j] // 2
    return D


def reference(D, col0, v0):
    """Per instance the reference's (col, u, v, cost, kept); an infeasible
    instance gets the cold entries' outputs and kept None (unspecified unless
    the prologue itself saw it)."""
    Dh = host(D)
    col0, v0 = col0.cpu().numpy(), v0.cpu().numpy()
    out = []
    for b in range(Dh.shape[0]):
        nr, nc = Dh[b].shape
        try:
            col, u, v, kept, searches = W.warm(Dh[b], col0[b], v0[b])
            assert searches == nr - kept
            out.append((col, u, v, Dh[b][np.arange(nr), col].sum(), kept))
        except ValueError:
            out.append((-np.ones(nr, dtype=np.int64), np.full(nr, np.nan), np.full(nc, np.nan), 0, None))
    return out


def check_against_reference(sh, D, col0, v0, flags=0, certify=True):
    ddt = torch.float64 if D.is_floating_point() else torch.int64
    B, nr, nc = D.shape
    before = (col0.clone(), v0.clone())
    col, cost, u, v, kept = sh.resolve_batched(D, col0, torch.zeros((B, nr), dtype=ddt, device="cuda"), v0, flags=flags)
    assert torch.equal(col0, before[0]) and same(v0.cpu().numpy(), before[1].cpu().numpy()), "inputs were modified"
    assert col.dtype == torch.int32 and kept.dtype == torch.int32 and cost.dtype == u.dtype == v.dtype == ddt
    ref = reference(D, col0, v0)
    for b, (rc, ru, rv, rcost, rkept) in enumerate(ref):
        assert same(col[b].cpu().numpy(), rc), b
        assert same(u[b].cpu().numpy(), ru), b
        assert same(v[b].cpu().numpy(), rv), b
        assert cost[b].item() == rcost, b
        assert rkept is None or int(kept[b]) == rkept, b
    if certify:
        fl = sh.check_duals_large(D, col, u, v)[3]
        assert fl.cpu().tolist() == [0] * B
    return col, cost, u, v, kept


# --------------------------------------------------------------------------- the prologue alone
PROLOGUE = [(dt, nr, nc) for dt in ("int64", "float64") for nr, nc in ((65, 65), (58, 65), (250, 257), (1018, 1025))]


@pytest.mark.parametrize("dtype,nr,nc", PROLOGUE, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in PROLOGUE])
def test_prologue_alone_equals_the_reference_entry_by_entry(sh, dtype, nr, nc):
    B = 3
    Ct = costs(dtype, B, nr, nc, 1)
    col, _, _, v = cold_state(sh, Ct)
    rng = np.random.default_rng([11, nr, nc])
    D = perturb(Ct, col, rng)
    garb_col = torch.from_numpy(rng.integers(-5, nc + 5, size=(B, nr))).cuda()
    garb_v = torch.from_numpy(rng.integers(-(1 << 19), 1 << 17, size=(B, nc))).to(v.dtype).cuda()
    for col0, v0 in ((col, v), (garb_col, garb_v), (col, garb_v), (garb_col, v)):
        gc, gcost, gu, gv, gkept = sh.resolve_batched(D, col0, torch.zeros_like(v[:, :nr]), v0, flags=SH_FLAG_BUILD_ONLY)
        Dh = host(D)
        for b in range(B):
            c4r, r4c, u, vv, kept = W.prologue(Dh[b], col0[b].cpu().numpy(), v0[b].cpu().numpy())
            assert same(gc[b].cpu().numpy(), c4r) and same(gu[b].cpu().numpy(), u) and same(gv[b].cpu().numpy(), vv)
            assert int(gkept[b]) == kept
        assert not gcost.any()


# --------------------------------------------------------------------------- the full warm solve
def sweep():
    for nc in SIZES:
        for nr in (nc, nc - 7):
            for dtype in ("int64", "float64"):
                yield dtype, nr, nc


SWEEP = list(sweep())


@pytest.mark.parametrize("dtype,nr,nc", SWEEP, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in SWEEP])
def test_warm_solve_equals_the_reference_and_certifies(sh, dtype, nr, nc):
    B = 2 if nc > 1025 else 3
    hi = 1 << 9 if (nr < nc and nc > 2049) else 1 << 20
    Ct = costs(dtype, B, nr, nc, 2, hi)
    col, _, _, v = cold_state(sh, Ct)
    D = perturb(Ct, col, np.random.default_rng([12, nr, nc]))
    _, _, _, _, kept = check_against_reference(sh, D, col, v)
    if nr == nc:  # one changed entry costs at most one pair
        assert int(kept.min()) >= nr - 3


NARROW_CASES = [(dt, nr, nc) for dt in NARROW for nc in (65, 257, 1025) for nr in (nc, nc - 7)]


@pytest.mark.parametrize("dtype,nr,nc", NARROW_CASES, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in NARROW_CASES])
def test_narrow_dtypes_on_integer_valued_costs(sh, dtype, nr, nc):
    Ct = costs(dtype, 3, nr, nc, 3, 64)  # [0, 64): exact in every dtype and in every sum
    col, _, _, v = cold_state(sh, Ct)
    D = perturb(Ct, col, np.random.default_rng([13, nr, nc]))
    assert same(host(D), np.round(host(D))) and float(host(D).min()) >= 0 and float(host(D).max()) < 128
    check_against_reference(sh, D, col, v)


def test_fractional_float64_costs_against_the_reference(sh):
    rng = np.random.default_rng(14)
    for nr, nc in ((65, 65), (250, 257)):
        Ct = torch.from_numpy(rng.random((3, nr, nc)) * 100.0).cuda()
        col, _, _, v = sh.solve_batched_large(Ct, duals=True)
        D = Ct.clone()
        for b in range(3):
            i = int(rng.integers(0, nr))
            D[b, i, int(col[b, i])] += 3.25
            D[b, (i + 1) % nr, int(rng.integers(0, nc))] = 0.0
        B = 3
        gc, gcost, gu, gv, gkept = sh.resolve_batched(D, col, torch.zeros_like(v[:, :nr]), v)
        Dh = D.cpu().numpy()
        for b in range(B):
            rc, ru, rv, rkept, _ = W.warm(Dh[b], col[b].cpu().numpy(), v[b].cpu().numpy())
            assert same(gc[b].cpu().numpy(), rc) and same(gu[b].cpu().numpy(), ru) and same(gv[b].cpu().numpy(), rv)
            assert int(gkept[b]) == rkept
            chosen = Dh[b][np.arange(nr), rc]
            # a fixed-order float64 sum of nr <= nc terms against numpy's: nc * 2^-53 * sum|chosen| each side
            assert abs(float(gcost[b]) - float(chosen.sum())) <= 2 * nc * 2.0 ** -53 * float(np.abs(chosen).sum())


# --------------------------------------------------------------------------- fixed point
FIXED = [(dt, nr, nc) for dt in ("int64", "float64", "float32", "int32")
         for nr, nc in ((64, 64), (58, 65), (257, 257), (1018, 1025), (2042, 2049))]


@pytest.mark.parametrize("dtype,nr,nc", FIXED, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in FIXED])
def test_a_solution_is_a_fixed_point(sh, dtype, nr, nc):
    Ct = costs(dtype, 2, nr, nc, 4, 64 if dtype in NARROW else 1 << 20)
    col, cost, u, v = cold_state(sh, Ct)
    wc, wcost, wu, wv, kept = sh.resolve_batched(Ct, col, u, v)
    assert kept.cpu().tolist() == [nr, nr]
    assert torch.equal(wc, col) and torch.equal(wcost, cost)
    assert torch.equal(wu, u) and torch.equal(wv, v)


# --------------------------------------------------------------------------- garbage
GARBAGE = [(dt, nr, nc) for dt in ("int64", "float64") for nr, nc in ((64, 64), (58, 65), (257, 257), (506, 513), (1018, 1025))]


@pytest.mark.parametrize("dtype,nr,nc", GARBAGE, ids=[f"{d}-{nr}x{nc}" for d, nr, nc in GARBAGE])
def test_a_garbage_state_is_data(sh, dtype, nr, nc):
    B = 3
    Ct = costs(dtype, B, nr, nc, 5)
    rng = np.random.default_rng([15, nr, nc])
    col0 = torch.from_numpy(rng.integers(-5, nc + 5, size=(B, nr))).cuda()  # out of range, duplicates
    if is_float(dtype):
        v0 = np.round(rng.normal(0.0, 1 << 18, size=(B, nc)))  # (integers: the certificate's arithmetic stays exact)
        v0[rng.random((B, nc)) < 0.1] = np.nan
        v0[rng.random((B, nc)) < 0.1] = np.inf
        v0[rng.random((B, nc)) < 0.1] = -np.inf
    else:
        v0 = rng.integers(-(1 << 19), 1 << 19, size=(B, nc))
        v0[rng.random((B, nc)) < 0.1] = -(1 << 56) - 1  # below the window
        v0[rng.random((B, nc)) < 0.1] = np.iinfo(np.int64).min
        v0[rng.random((B, nc)) < 0.05] = -(1 << 56)  # its edge: a dual
    check_against_reference(sh, Ct, col0, torch.from_numpy(v0).cuda())


# --------------------------------------------------------------------------- the empty state: a full solve
def empty_state(B, nr, nc, ddt):
    return (torch.full((B, nr), -1, dtype=torch.int16, device="cuda"), torch.zeros((B, nc), dtype=ddt, device="cuda"))


@pytest.mark.parametrize("dtype", ("int64", "float64"))
@pytest.mark.parametrize("nr,nc", ((128, 128), (100, 128)))
def test_empty_state_on_machol_wien_equals_the_reference(sh, dtype, nr, nc):
    Ct = torch.from_numpy(F.make("mw", "int64", nr, nc)[None]).to(TORCH[dtype]).cuda()
    col0, v0 = empty_state(1, nr, nc, torch.float64 if is_float(dtype) else torch.int64)
    a = check_against_reference(sh, Ct, col0, v0)
    b = check_against_reference(sh, Ct, col0, v0, flags=SH_FLAG_EXACT_ARGMIN)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[4].tolist() == [0]


EMPTY = [(dt, fam, n) for dt in ("int64", "float64") for fam, n in (("mw", 513), ("mw", 1025), ("rand", 2049), ("rand", 3073), ("rand", 4096))]


@pytest.mark.parametrize("dtype,family,n", EMPTY, ids=[f"{d}-{f}-{n}" for d, f, n in EMPTY])
def test_empty_state_is_a_full_solve_with_the_cold_cost(sh, dtype, family, n):
    if family == "mw":  # long searches from u = the row minima through the windowed keys
        Ct = torch.from_numpy(F.make("mw", "int64", n, n)[None]).to(TORCH[dtype]).cuda()
    else:
        Ct = costs(dtype, 2, n, n, 6)
    B = Ct.shape[0]
    ccol, ccost, _, _ = cold_state(sh, Ct)
    ddt = ccost.dtype
    col0, v0 = empty_state(B, n, n, ddt)
    out = [sh.resolve_batched(Ct, col0, torch.zeros((B, n), dtype=ddt, device="cuda"), v0, flags=fl)
           for fl in ((0, SH_FLAG_EXACT_ARGMIN) if dtype == "int64" else (0,))]
    for col, cost, u, v, kept in out:
        assert not kept.any() and torch.equal(cost, ccost)
        assert sh.check_duals_large(Ct, col, u, v)[3].cpu().tolist() == [0] * B
        assert torch.equal(col, out[0][0]) and torch.equal(u, out[0][2]) and torch.equal(v, out[0][3])


# --------------------------------------------------------------------------- int64 extremes
@pytest.mark.parametrize("nr,nc", ((65, 65), (58, 65), (257, 257), (1025, 1025), (1018, 1025), (1500, 2049)))
def test_int64_extremes_with_the_duals_at_the_window_edge(sh, nr, nc):
    from santa_hip.lsap import int64_cost_limit
    top = int64_cost_limit(nc) - 1
    rng = np.random.default_rng([16, nr, nc])
    B = 2
    C = np.where(rng.random((B, nr, nc)) < 0.5, top, -top).astype(np.int64)
    C[0] -= np.sign(C[0]) * rng.integers(0, 1 << 20, size=(nr, nc))  # (instance 1: nothing but the two extremes)
    Ct = torch.from_numpy(C).cuda()
    col0 = torch.from_numpy(np.stack([rng.permutation(nc)[:nr] for _ in range(B)])).cuda()
    v0 = torch.full((B, nc), -(1 << 56), dtype=torch.int64, device="cuda")
    v0[:, ::5] = 0
    u0 = torch.zeros((B, nr), dtype=torch.int64, device="cuda")
    if nc <= 257:
        col, cost, u, v, kept = check_against_reference(sh, Ct, col0, v0)
    else:
        col, cost, u, v, kept = sh.resolve_batched(Ct, col0, u0, v0)
    smin, tmax, gap, fl = sh.check_duals_large(Ct, col, u, v)
    assert fl.cpu().tolist() == [0] * B  # in particular no SH_CERT_RANGE
    ccost = sh.solve_batched_large(Ct)[1]
    assert torch.equal(cost, ccost)


# --------------------------------------------------------------------------- ragged batches
def raw_warm(sh, Ct, shapes, col, u, v, kept, cost):
    """The C entry itself: resolve_batched refuses an invalid shape on the host."""
    from santa_hip import _lib
    from santa_hip.lsap import DTYPE_SUFFIX
    B, NR, NC = Ct.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = getattr(_lib.lib(), "lsap_warm_" + DTYPE_SUFFIX[Ct.dtype])(p(Ct), NR, NC, B, p(shapes), p(col), p(cost), p(u), p(v),
                                                                   p(kept), 0, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()


@pytest.mark.parametrize("dtype", ("int64", "float64", "float32"))
def test_ragged_batch_with_an_empty_and_an_invalid_shape(sh, dtype):
    NR, NC = 70, 80
    shapes = [(70, 80), (0, 0), (64, 64), (9, 5), (33, 80), (71, 80), (1, 1), (65, 70)]  # (9, 5) tall, (71, 80) too many rows
    B = len(shapes)
    flt = is_float(dtype)
    ddt = torch.float64 if flt else torch.int64
    rng = np.random.default_rng(17)
    C = rng.integers(0, 1 << 16, size=(B, NR, NC)).astype(np.float64 if flt else np.int64)
    live = np.zeros((B, NR, NC), dtype=bool)
    ok = [0 < nr <= nc <= NC and nr <= NR for nr, nc in shapes]
    for b, (nr, nc) in enumerate(shapes):
        if ok[b]:
            live[b, :nr, :nc] = True
    C[~live] = np.nan if flt else -(1 << 40)  # the padding is never read
    Ct = torch.from_numpy(C).to(TORCH[dtype]).cuda()
    col0 = rng.integers(-3, NC + 3, size=(B, NR)).astype(np.int32)
    v0 = -rng.integers(0, 1 << 15, size=(B, NC)).astype(np.float64 if flt else np.int64)
    col = torch.from_numpy(col0).cuda()
    v = torch.from_numpy(v0).cuda()
    u = torch.full((B, NR), 7, dtype=ddt, device="cuda")
    kept = torch.full((B,), -9, dtype=torch.int32, device="cuda")
    cost = torch.full((B,), 7, dtype=ddt, device="cuda")
    raw_warm(sh, Ct, torch.tensor(shapes, dtype=torch.int32, device="cuda"), col, u, v, kept, cost)
    col, u, v, kept, cost = (t.cpu().numpy() for t in (col, u, v, kept, cost))
    for b, (nr, nc) in enumerate(shapes):
        if not ok[b]:
            assert (col[b] == -1).all() and not u[b].any() and not v[b].any() and kept[b] == 0 and cost[b] == 0, b
            continue
        Dh = C[b, :nr, :nc]
        rc, ru, rv, rkept, _ = W.warm(Dh, col0[b, :nr], v0[b, :nc])
        assert same(col[b, :nr], rc) and (col[b, nr:] == -1).all(), b
        assert same(u[b, :nr], ru) and not u[b, nr:].any(), b
        assert same(v[b, :nc], rv) and not v[b, nc:].any(), b
        assert kept[b] == rkept and cost[b] == Dh[np.arange(nr), rc].sum(), b
        assert all(R.invariants(Dh.astype(np.int64), rc, ru.astype(np.int64), rv.astype(np.int64)).values()), b
    # the valid shapes through the front end: the same results
    keep = [b for b in range(B) if ok[b] or shapes[b] == (0, 0)]
    fc, fcost, fu, fv, fkept = sh.resolve_batched(Ct[keep], torch.from_numpy(col0[keep]).cuda(), torch.zeros((len(keep), NR), dtype=ddt, device="cuda"),
                                                  torch.from_numpy(v0[keep]).cuda(), shapes=[shapes[b] for b in keep])
    assert same(fc.cpu().numpy(), col[keep]) and same(fu.cpu().numpy(), u[keep]) and same(fv.cpu().numpy(), v[keep])
    assert same(fkept.cpu().numpy(), kept[keep]) and same(fcost.cpu().numpy(), cost[keep])


# --------------------------------------------------------------------------- float infeasibility
@pytest.mark.parametrize("dtype", ("float64", "float32"))
@pytest.mark.parametrize("nr,nc", ((64, 64), (60, 65), (300, 300)))
def test_float_infeasibility(sh, dtype, nr, nc):
    Ct = costs(dtype, 3, nr, nc, 8, 64)
    col, _, _, v = cold_state(sh, Ct)
    D = Ct.clone()
    D[0, 5, :] = float("inf")  # a row of +inf: the prologue sees it
    # instance 1: rows 2 and 3 can only take the column row 2 held: no perfect matching is left
    j = int(col[1, 2])
    keepcol = D[1, 2:4, j].clone()
    D[1, 2:4, :] = float("inf")
    D[1, 2:4, j] = keepcol
    gc, gcost, gu, gv, gkept = check_against_reference(sh, D, col, v, certify=False)
    for b in (0, 1):
        assert bool((gc[b] == -1).all()) and float(gcost[b]) == 0.0
        assert bool(torch.isnan(gu[b]).all()) and bool(torch.isnan(gv[b]).all())
    assert int(gkept[0]) == 0
    assert bool((gc[2] >= 0).all())  # the feasible neighbour is solved
    cold = sh.solve_batched_large(D, duals=True)
    assert torch.equal(gc[:2], cold[0][:2]) and torch.equal(gcost, cold[1])
    with pytest.raises(ValueError, match="infeasible"):
        sh.linear_sum_assignment_resolve(host(D[1]), col[1].cpu().numpy(), np.zeros(nr), v[1].cpu().numpy())


# --------------------------------------------------------------------------- the Python surface
@pytest.mark.parametrize("dtype", ("int64", "float64"))
def test_a_tall_batch_is_solved_as_its_transpose(sh, dtype):
    NR, NC, B = 65, 64, 3
    Ct = costs(dtype, B, NR, NC, 9)
    col, cost, u, v = sh.solve_batched_large(Ct, duals=True)
    assert not sh.check_duals_large(Ct, col, u, v)[3].any()
    rng = np.random.default_rng(18)
    D = Ct.clone()
    for b in range(B):
        D[b, int(rng.integers(0, NR)), int(rng.integers(0, NC))] = 0
    col0 = col.clone()
    col0[2, :] = 3  # no partial assignment: instance 2 starts from the empty matching
    wc, wcost, wu, wv, kept = sh.resolve_batched(D, col0.long(), u, v)
    assert tuple(wc.shape) == (B, NR) and tuple(wu.shape) == (B, NR) and tuple(wv.shape) == (B, NC)
    assert not sh.check_duals_large(D, wc, wu, wv)[3].any()
    assert torch.equal(wcost, sh.solve_batched_large(D)[1])
    assert int(kept[2]) == 0
    # the reference on the transpose: u plays v0, col its inverse
    Dh = host(D)
    for b in range(B):
        inv = -np.ones(NC, dtype=np.int64)
        if b != 2:
            c = col[b].cpu().numpy()
            inv[c[c >= 0]] = np.flatnonzero(c >= 0)
        rc, ru, rv, rkept, _ = W.warm(Dh[b].T, inv, u[b].cpu().numpy())
        back = -np.ones(NR, dtype=np.int64)
        back[rc] = np.arange(NC)
        assert same(wc[b].cpu().numpy(), back) and same(wu[b].cpu().numpy(), rv) and same(wv[b].cpu().numpy(), ru)
        assert int(kept[b]) == rkept


@pytest.mark.parametrize("dtype", ("int32", "float64"))
def test_maximize(sh, dtype):
    B, nr, nc = 3, 60, 65
    Ct = costs(dtype, B, nr, nc, 10, 1 << 16)
    col, cost, u, v = sh.solve_batched_large(Ct, maximize=True, duals=True)
    D = perturb(Ct, col, np.random.default_rng(19))
    wc, wcost, wu, wv, kept = sh.resolve_batched(D, col, u, v, maximize=True)
    assert not sh.check_duals_large(D, wc, wu, wv, maximize=True)[3].any()
    assert torch.equal(wcost, sh.solve_batched_large(D, maximize=True)[1])
    Dh = -host(D)
    for b in range(B):
        rc, ru, rv, rkept, _ = W.warm(Dh[b], col[b].cpu().numpy(), -v[b].cpu().numpy())
        assert same(wc[b].cpu().numpy(), rc) and same(wu[b].cpu().numpy(), -ru) and same(wv[b].cpu().numpy(), -rv)
        assert int(kept[b]) == rkept


@pytest.mark.parametrize("shape", ((40, 40), (30, 45), (45, 30)))
@pytest.mark.parametrize("kind", ("int", "float"))
def test_single_matrix_front_end_reaches_the_optimum(sh, shape, kind):
    scipy_opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng([20, *shape])
    C = rng.integers(0, 1000, size=shape)
    if kind == "float":
        C = C + rng.integers(0, 4, size=shape) * 0.25
    for maximize in (False, True):
        r0, c0, u0, v0 = sh.linear_sum_assignment_large(C, maximize=maximize, duals=True)
        D = C.copy()
        D[3, 7] = 0
        D[r0[5], c0[5]] += 50
        prev = np.full(shape[0], -1, dtype=np.int64)
        prev[r0] = c0
        r, c, u, v = sh.linear_sum_assignment_resolve(D, prev, u0, v0, maximize=maximize)
        sr, sc = scipy_opt.linear_sum_assignment(D, maximize=maximize)
        assert len(r) == min(shape) and (np.diff(r) > 0).all() and len(set(c.tolist())) == len(c)
        if shape[0] <= shape[1]:
            assert np.array_equal(r, sr)
        assert D[r, c].sum() == D[sr, sc].sum()
        slack = D - u[:, None] - v[None, :]
        assert (slack <= 0).all() if maximize else (slack >= 0).all()
        assert (slack[r, c] == 0).all()
