"""GPU tests of the batched LSAP above 1024 columns: solve_batched_large,
check_duals_large and linear_sum_assignment_large (the lsap_*_large_ entries).

Every instance is compared with the CPU oracle for equal columns; integer
costs for equality, float costs against the rounding bound of a fixed-order
sum and bit for bit between storage dtypes of the same values.  Integer duals
are certified on the device (check_duals_large's flags == 0 proves an instance
optimal) and, on the wide shapes, compared with the CPU replay of scipy's loop;
float duals are compared with the replay bit for bit.  The cases, shapes and
batch sizes are lsap_large_families'; the Machol-Wien replays come from
tests/golden/lsap_large_replay.npz."""
import functools
import json
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_duals_ref as R  # noqa: E402
import lsap_families as F  # noqa: E402
import lsap_large_families as L  # noqa: E402
import oracle  # noqa: E402
from conftest import GOLDEN, load_npz_cases  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_EXACT_ARGMIN = 2
SH_FLAG_F64_MW = 16384
SH_FLAG_F64_SW = 32768
INT_FLAGS = (0, SH_FLAG_EXACT_ARGMIN)
F64_FLAGS = (0, SH_FLAG_F64_MW)
COL, SLACK, TIGHT, SIGN, GAP, NONE, RANGE = 1, 2, 4, 8, 16, 32, 64


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("solve_batched_large", "check_duals_large", "linear_sum_assignment_large"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    """float64 arrays equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def oracle_col(C):
    """oracle.lsap's columns of one wide matrix, -1 everywhere when infeasible."""
    try:
        return oracle.lsap(C)[1]
    except ValueError:
        return -np.ones(C.shape[0], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _recorded():
    z = np.load(os.path.join(GOLDEN, "lsap_large_replay.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    return {tuple(m["key"]): (m["sha"], z[f"col{i}"], z[f"u{i}"], z[f"v{i}"]) for i, m in enumerate(meta)}


@functools.lru_cache(maxsize=None)
def replay_instance(family, dtype, nr, nc, k):
    """lsap_duals_ref.replay of an instance: recorded for the Machol-Wien
    cases (the matrix must still hash to what was recorded), computed
    otherwise; NaN duals and -1 for an infeasible one."""
    C = L.instance(family, dtype, nr, nc, k)
    key = (family, dtype, nr, nc, k)
    if key in _recorded():
        sha, col, u, v = _recorded()[key]
        assert sha == F.matrix_sha(C), f"{key}: the matrix changed, rewrite lsap_large_replay.npz"
        return col.astype(np.int64), u, v
    try:
        return R.replay(C)
    except ValueError:
        return -np.ones(nr, dtype=np.int64), np.full(nr, np.nan), np.full(nc, np.nan)


@functools.lru_cache(maxsize=None)
def batch(family, dtype, nr, nc):
    """(C [B, nr, nc], the oracle's columns [B, nr]) of a case, computed once."""
    B = L.batch_size(nr, nc)
    C = np.stack([L.instance(family, dtype, nr, nc, k) for k in range(B)])
    return C, np.stack([oracle_col(C[k]) for k in range(B)])


def replay_batch(family, dtype, nr, nc):
    rep = [replay_instance(family, dtype, nr, nc, k) for k in range(L.batch_size(nr, nc))]
    return np.stack([r[0] for r in rep]), np.stack([r[1] for r in rep]), np.stack([r[2] for r in rep])


def check_cost_bound(C64, col, cost, nc):
    """|cost - exact sum| <= nc * 2^-53 * sum|chosen| for a fixed-order sum of
    nr <= nc terms (test_lsap_adversarial_gpu's bound); cost 0 where no
    assignment exists."""
    for b in range(C64.shape[0]):
        if (col[b] < 0).any():
            assert float(cost[b]) == 0.0, b
            continue
        chosen = C64[b, np.arange(C64.shape[1]), col[b]]
        exact = math.fsum(chosen.tolist())
        bound = nc * 2.0 ** -53 * math.fsum(np.abs(chosen).tolist())
        print(f"cost[{b}] = {float(cost[b])!r}, exact {exact!r}, bound {bound!r}")
        assert abs(float(cost[b]) - exact) <= bound, (b, float(cost[b]), exact)


# --------------------------------------------------------------------------- integer
INT_CASES = [(f, nr, nc, "int64") for f, nr, nc in L.int_cases()]
INT_CASES += [(f, nr, nc, "int32") for f, nr, nc in L.int_cases() if f in L.INT32_FAMILIES]


@pytest.mark.parametrize("family,nr,nc,dtype", INT_CASES, ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in INT_CASES])
def test_integer_solves_match_the_oracle_and_certify(sh, family, nr, nc, dtype):
    C, ocol = batch(family, "int64", nr, nc)
    B = C.shape[0]
    Ct = torch.from_numpy(C).cuda()
    if dtype == "int32":
        Ct = Ct.to(torch.int32)
        assert torch.equal(Ct.cpu().long(), torch.from_numpy(C))  # (the family fits int32)
    want_cost = np.array([int(C[b, np.arange(nr), ocol[b]].sum()) for b in range(B)])
    for flags in INT_FLAGS:
        col, cost, u, v = sh.solve_batched_large(Ct, flags=flags, duals=True)
        assert col.dtype == torch.int32 and cost.dtype == u.dtype == v.dtype == torch.int64
        assert np.array_equal(col.cpu().numpy(), ocol), (family, nr, nc, dtype, flags)
        assert np.array_equal(cost.cpu().numpy(), want_cost), (family, nr, nc, dtype, flags)
        if flags == 0:  # the kernel without duals returns the same
            col0, cost0 = sh.solve_batched_large(Ct)
            assert torch.equal(col, col0) and torch.equal(cost, cost0)
        smin, tmax, gap, fl = sh.check_duals_large(Ct, col, u, v)
        assert fl.cpu().tolist() == [0] * B, (family, nr, nc, dtype, flags, fl.cpu().tolist())
        assert smin.dtype == torch.int64 and bool((smin >= 0).all()) and not tmax.any() and not gap.any()
        if (nr, nc) in L.WIDE:
            rcol, ru, rv = replay_batch(family, "int64", nr, nc)
            assert np.array_equal(rcol, ocol)
            assert np.array_equal(u.cpu().numpy(), ru) and np.array_equal(v.cpu().numpy(), rv), (family, nr, nc, flags)


def test_the_window_families_leave_the_12_bit_window(sh):
    """The steps the families aim outside [WINDOW_LO12, WINDOW_HI12) are there:
    lsap_families.sap_trace of a short instance of each names them."""
    for family, above, below in (("window_edges12", True, True), ("two_scale38", True, False),
                                 ("two_scale41", True, False), ("neg_cols", False, True)):
        _, d, first, _ = F.sap_trace(L.instance(family, "int64", 40, 1100, 0))
        assert (d >= L.WINDOW_HI12).any() == above and (d < L.WINDOW_LO12).any() == below, family
    _, d, _, _ = F.sap_trace(L.instance("window_edges12", "int64", 14, 1100, 0))
    assert {L.WINDOW_HI12 - 1, L.WINDOW_HI12, L.WINDOW_LO12 - 1, L.WINDOW_LO12} <= set(d.tolist())


# --------------------------------------------------------------------------- float
F64_CASES = [(f, nr, nc, "float64") for f, nr, nc in L.float_cases()]
F64_CASES += [(f, nr, nc, d) for f, nr, nc in L.float_cases() for d in sorted(F.NARROW)]


@functools.lru_cache(maxsize=2)
def f64_result(family, nr, nc):
    """What the float64 kernel returned for a case (flags 0), as numpy: the
    narrow dtypes of the same values must return these bits."""
    import santa_hip
    C, _ = batch(family, "float64", nr, nc)
    out = santa_hip.solve_batched_large(torch.from_numpy(C).cuda(), duals=True)
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("family,nr,nc,dtype", F64_CASES, ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in F64_CASES])
def test_float_solves_match_the_oracle_and_the_replays_bits(sh, family, nr, nc, dtype):
    """float64: columns the oracle's, cost within the summation bound, duals
    the replay's bits, with the default kernel and SH_FLAG_F64_MW.  A narrow
    dtype holds the float64 matrix rounded to it: its solve returns, bit for
    bit, what the float64 kernel returns for the widened values, and the
    oracle's columns; where the rounding is exact (tiny_range, inf_band) those
    are the float64 case's bits and the replay's."""
    C64, ocol = batch(family, "float64", nr, nc)
    B = C64.shape[0]
    exact = True
    if dtype == "float64":
        Cd = torch.from_numpy(C64).cuda()
    else:
        Cn = L.narrow(C64, F.NARROW[dtype])
        W64 = Cn.double().numpy()
        exact = np.array_equal(W64, C64)
        assert exact == (family != "mw_tenths")
        if not exact:
            C64, ocol = W64, np.stack([oracle_col(W64[k]) for k in range(B)])
        Cd = Cn.cuda()
    feasible = (ocol >= 0).all(axis=1)
    assert feasible.all() or dtype == "float16"  # (float16 Machol-Wien rows overflow to +inf)
    got = []
    for flags in F64_FLAGS:
        col, cost, u, v = sh.solve_batched_large(Cd, flags=flags, duals=True)
        assert col.dtype == torch.int32 and cost.dtype == u.dtype == v.dtype == torch.float64
        assert np.array_equal(col.cpu().numpy(), ocol), (family, nr, nc, dtype, flags)
        got.append((col, cost, u, v))
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a if a.dtype == torch.int32 else bits(a), b if b.dtype == torch.int32 else bits(b))
    col, cost, u, v = got[0]
    col0, cost0 = sh.solve_batched_large(Cd)
    assert torch.equal(col, col0) and torch.equal(bits(cost), bits(cost0))
    check_cost_bound(C64, ocol, cost.cpu().numpy(), nc)
    un, vn = u.cpu().numpy(), v.cpu().numpy()
    for b in range(B):
        if not feasible[b]:
            assert np.isnan(un[b]).all() and np.isnan(vn[b]).all()
    if exact:
        rcol, ru, rv = replay_batch(family, "float64", nr, nc)
        assert np.array_equal(rcol, ocol)
        assert same_bits(un, ru) and same_bits(vn, rv), (family, nr, nc, dtype)
    if dtype != "float64":
        if exact:
            wcol, wcost, wu, wv = f64_result(family, nr, nc)
        else:
            wcol, wcost, wu, wv = (t.cpu().numpy() for t in
                                   sh.solve_batched_large(torch.from_numpy(C64).cuda(), duals=True))
        assert np.array_equal(col.cpu().numpy(), wcol) and same_bits(cost.cpu().numpy(), wcost)
        assert same_bits(un, wu) and same_bits(vn, wv), (family, nr, nc, dtype)
    fl = sh.check_duals_large(Cd, col, u, v)[3].cpu().tolist()
    for b in range(B):
        assert fl[b] == NONE if not feasible[b] else not fl[b] & (COL | NONE | GAP | RANGE), (b, fl[b])


@pytest.mark.parametrize("dtype", ["float64"] + sorted(F.NARROW))
def test_infeasible_float_instance(sh, dtype):
    """One instance of three has a row of +inf: -1 everywhere, cost 0, NaN
    duals, SH_CERT_NONE; its neighbours are solved."""
    family, nr, nc = L.INFEASIBLE_CASE
    C = np.stack([L.instance("inf_band", "float64", nr, nc, 0), L.instance(family, "float64", nr, nc, 1),
                  L.instance("inf_band", "float64", nr, nc, 2)])
    Cd = torch.from_numpy(C).cuda() if dtype == "float64" else L.narrow(C, F.NARROW[dtype]).cuda()
    assert np.array_equal(Cd.double().cpu().numpy(), C)
    for flags in F64_FLAGS:
        col, cost, u, v = sh.solve_batched_large(Cd, flags=flags, duals=True)
        col0, cost0 = sh.solve_batched_large(Cd, flags=flags)
        assert torch.equal(col, col0) and torch.equal(bits(cost), bits(cost0))
        assert bool((col[1] == -1).all()) and float(cost[1]) == 0.0
        assert bool(torch.isnan(u[1]).all()) and bool(torch.isnan(v[1]).all())
        for b in (0, 2):
            rc, ru, rv = replay_instance("inf_band", "float64", nr, nc, b)
            assert np.array_equal(col[b].cpu().numpy(), rc)
            assert same_bits(u[b].cpu().numpy(), ru) and same_bits(v[b].cpu().numpy(), rv)
        fl = sh.check_duals_large(Cd, col, u, v)[3].cpu().tolist()
        assert fl[1] == NONE and not (fl[0] | fl[2]) & (NONE | COL)
    with pytest.raises(ValueError, match="infeasible"):
        sh.linear_sum_assignment_large(C[1])


def test_one_wave_flag_is_refused_above_1024_columns(sh):
    C = torch.zeros((1, 2, 1025), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="one-wave"):
        sh.solve_batched_large(C, flags=SH_FLAG_F64_SW)
    with pytest.raises(ValueError, match="exclude"):
        sh.solve_batched_large(C, flags=SH_FLAG_F64_SW | SH_FLAG_F64_MW)


# --------------------------------------------------------------------------- the certificate above column 1023
def test_certificate_names_corruptions_above_index_1023(sh):
    """A unique optimum by construction: C[i][j] = 1000 + noise except a
    planted cheap entry per row at column p[i] >= 1024."""
    nr, nc, B = 1100, 2500, 2
    rng = np.random.default_rng(99)
    C = rng.integers(1000, 2000, size=(B, nr, nc), dtype=np.int64)
    p = np.stack([1024 + rng.permutation(nc - 1024)[:nr] for _ in range(B)])
    for b in range(B):
        C[b, np.arange(nr), p[b]] = rng.integers(0, 10, size=nr)
    Cd = torch.from_numpy(C).cuda()
    col, cost, u, v = sh.solve_batched_large(Cd, duals=True)
    assert np.array_equal(col.cpu().numpy(), p)  # (any other entry costs 1000 more than it can save)
    assert sh.check_duals_large(Cd, col, u, v)[3].cpu().tolist() == [0, 0]

    def flags_of(b, col=col, u=u, v=v):
        fl = sh.check_duals_large(Cd, col, u, v)[3].cpu().tolist()
        assert all(f == 0 for k, f in enumerate(fl) if k != b), fl
        return fl[b]

    x = u.clone()
    x[1, 1050] += 1  # row 1050's chosen entry now has slack -1
    assert flags_of(1, u=x) == SLACK | TIGHT | GAP
    x = u.clone()
    x[0, 1099] -= 1  # feasible, no longer tight
    assert flags_of(0, u=x) == TIGHT | GAP
    x = col.clone()
    x[1, 1030], x[1, 1090] = col[1, 1090], col[1, 1030]  # another assignment: dearer, the optimum being unique
    f = flags_of(1, col=x)
    assert f & TIGHT and not f & (COL | SLACK | SIGN | NONE | RANGE)
    x = col.clone()
    x[0, 1025] = col[0, 1026]  # one column (>= 1024) taken twice
    assert flags_of(0, col=x) & COL
    x = col.clone()
    x[0, 1025] = nc  # outside [0, nc)
    assert flags_of(0, col=x) & COL
    free = sorted(set(range(1024, nc)) - set(p[1].tolist()))[-1]
    assert free >= 1024
    for bad in (1, -1):  # a free column must stay at 0
        x = v.clone()
        x[1, free] = bad
        assert flags_of(1, v=x) & SIGN
    x = v.clone()
    x[0, int(p[0, 7])] -= 1  # a taken column >= 1024: its entry is no longer tight
    assert flags_of(0, v=x) == TIGHT | GAP
    x = v.clone()
    x[0, int(p[0, 7])] += 1
    assert flags_of(0, v=x) & SLACK
    x = u.clone()
    x[1, 1080] = 1 << 61
    assert flags_of(1, u=x) & RANGE


# --------------------------------------------------------------------------- ragged, tall, maximize
RAGGED_SHAPES = [(0, 0), (1, 1), (1, 4096), (64, 64), (1000, 1024), (1025, 1025), (1500, 4096), (7, 3)]


@pytest.mark.parametrize("dtype", ["int64", "float64", "float32"])
def test_ragged_batch_reads_nothing_outside_its_corners(sh, dtype):
    """A batch padded [8, 1500, 4096]; the padding is a poison integer that
    would win every argmin, or NaN.  (7, 3) is no shape of a wide instance:
    -1, cost 0, zero duals, and SH_CERT_COL from the certificate."""
    NR, NC = 1500, 4096
    rng = np.random.default_rng(17)
    B = len(RAGGED_SHAPES)
    if dtype == "int64":
        C = np.full((B, NR, NC), -(1 << 47), dtype=np.int64)
        live = [rng.integers(-50, 50, size=s, dtype=np.int64) for s in RAGGED_SHAPES]
    else:
        C = np.full((B, NR, NC), np.nan, dtype=np.float64 if dtype == "float64" else np.float32)
        live = [rng.integers(0, 1 << 20, size=s).astype(C.dtype) for s in RAGGED_SHAPES]
    for b, (nr, nc) in enumerate(RAGGED_SHAPES[:-1]):
        C[b, :nr, :nc] = live[b]
    Cd = torch.from_numpy(C).cuda()
    # the front end refuses an invalid shape; the C-ABI entry answers it per instance
    with pytest.raises(ValueError, match="tall"):
        sh.solve_batched_large(Cd, shapes=RAGGED_SHAPES)
    from santa_hip import _lib, lsap
    ddt = torch.int64 if dtype == "int64" else torch.float64
    shape_dev = torch.tensor(RAGGED_SHAPES, dtype=torch.int32, device="cuda")
    col = torch.full((B, NR), 7, dtype=torch.int32, device="cuda")
    cost = torch.full((B,), 7, dtype=ddt, device="cuda")
    u = torch.full((B, NR), 7, dtype=ddt, device="cuda")
    v = torch.full((B, NC), 7, dtype=ddt, device="cuda")
    entry = getattr(_lib.lib(), "lsap_solve_large_" + lsap.DTYPE_SUFFIX[Cd.dtype])
    p = lsap._p
    _lib.check(entry(p(Cd), NR, NC, B, p(shape_dev), p(col), p(cost), p(u), p(v), 1,
                     lsap.current_stream_handle(Cd.device)), "lsap_solve_large")
    good = RAGGED_SHAPES[:-1]
    col2, cost2, u2, v2 = sh.solve_batched_large(Cd[:-1], shapes=good, duals=True)
    assert torch.equal(col[:-1], col2) and torch.equal(bits(cost[:-1]), bits(cost2))
    assert torch.equal(bits(u[:-1]), bits(u2)) and torch.equal(bits(v[:-1]), bits(v2))
    col3, cost3 = sh.solve_batched_large(Cd[:-1], shapes=good)
    assert torch.equal(col2, col3) and torch.equal(bits(cost2), bits(cost3))
    cn, un, vn = col.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()
    assert (cn[-1] == -1).all() and float(cost[-1]) == 0 and not un[-1].any() and not vn[-1].any()
    assert (cn[0] == -1).all() and float(cost[0]) == 0 and not un[0].any() and not vn[0].any()
    for b, (nr, nc) in enumerate(good):
        assert (cn[b, nr:] == -1).all() and not un[b, nr:].any() and not vn[b, nc:].any(), b
        assert not np.isnan(un[b].astype(np.float64)).any() and not np.isnan(vn[b].astype(np.float64)).any()
        if nr:
            want = oracle_col(live[b] if dtype == "int64" else live[b].astype(np.float64))
            assert np.array_equal(cn[b, :nr], want), (b, nr, nc)
            chosen = live[b][np.arange(nr), want]
            assert float(cost[b]) == float(chosen.astype(np.float64).sum()) if dtype != "int64" else \
                int(cost[b]) == int(chosen.sum())  # (integers below 2^20: every partial sum is exact)
    smin, tmax, gap, fl = sh.check_duals_large(Cd[:-1], col2, u2, v2, shapes=good)
    if dtype == "int64":
        assert fl.cpu().tolist() == [0] * len(good)
    else:
        assert not any(f & (COL | NONE | SIGN) for f in fl.cpu().tolist())
    assert not np.isnan(smin.cpu().numpy().astype(np.float64)).any()
    # the certificate entry on the invalid shape, and a padded row that claims a column
    slack = torch.zeros((B, 3), dtype=ddt, device="cuda")
    flg = torch.zeros(B, dtype=torch.int32, device="cuda")
    centry = getattr(_lib.lib(), "lsap_check_duals_large_" + lsap.DTYPE_SUFFIX[Cd.dtype])
    _lib.check(centry(p(Cd), NR, NC, B, p(shape_dev), p(col), p(u), p(v), p(slack), p(flg),
                      lsap.current_stream_handle(Cd.device)), "lsap_check_duals_large")
    assert flg.cpu().tolist()[:-1] == fl.cpu().tolist() and flg.cpu().tolist()[-1] == COL
    bad = col2.clone()
    bad[5, 1300] = 1030
    assert sh.check_duals_large(Cd[:-1], bad, u2, v2, shapes=good)[3].cpu().tolist()[5] & COL


@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_tall_batch_is_solved_as_its_transpose(sh, dtype):
    nr, nc, B = 4096, 300, 3
    rng = np.random.default_rng(41)
    C = rng.integers(-1000, 1000, size=(B, nr, nc), dtype=np.int64)
    if dtype == "float64":
        C = C * 0.25
    Cd = torch.from_numpy(C).cuda()
    col0, cost0 = sh.solve_batched_large(Cd)
    col, cost, u, v = sh.solve_batched_large(Cd, duals=True)
    assert torch.equal(col, col0) and torch.equal(bits(cost), bits(cost0))
    assert tuple(col.shape) == (B, nr) and tuple(u.shape) == (B, nr) and tuple(v.shape) == (B, nc)
    assert bool((u <= 0).all()) and bool((u[col < 0] == 0).all()) and int((col < 0).sum()) == B * (nr - nc)
    for b in range(B):
        wr, wc = oracle.lsap(C[b])
        got = col[b].cpu().numpy()
        assert np.array_equal(np.flatnonzero(got >= 0), wr) and np.array_equal(got[wr], wc)
        rc, ru, rv = R.replay(np.ascontiguousarray(C[b].T))  # the transposed solve's duals
        assert same_bits(u[b].cpu().numpy().astype(np.float64), rv.astype(np.float64))
        assert same_bits(v[b].cpu().numpy().astype(np.float64), ru.astype(np.float64))
    smin, tmax, gap, fl = sh.check_duals_large(Cd, col, u, v)
    if dtype == "int64":
        assert fl.cpu().tolist() == [0] * B and bool((smin >= 0).all())
    else:
        assert not any(f & (COL | NONE | SIGN | RANGE) for f in fl.cpu().tolist())
    dup = col.clone()
    i, k = [int(x) for x in torch.nonzero(col[1] >= 0)[-2:, 0]]
    dup[1, i] = dup[1, k]  # two rows on one column: found before the inversion
    fl = sh.check_duals_large(Cd, dup, u, v)[3].cpu().tolist()
    assert fl[1] & COL and not fl[0] & COL


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float32])
def test_maximize_on_a_wide_batch(sh, dtype):
    nr, nc, B = 300, 2049, 3
    Cn = np.random.default_rng(43).integers(-500, 500, size=(B, nr, nc))
    C = torch.from_numpy(Cn).to(dtype).cuda()
    col0, cost0 = sh.solve_batched_large(C, maximize=True)
    col, cost, u, v = sh.solve_batched_large(C, maximize=True, duals=True)
    assert torch.equal(col, col0) and torch.equal(bits(cost.double()), bits(cost0.double()))
    for b in range(B):
        assert np.array_equal(col[b].cpu().numpy(), oracle.lsap(-Cn[b].astype(np.float64 if dtype.is_floating_point
                                                                              else np.int64))[1])
        assert float(cost[b]) == float(Cn[b, np.arange(nr), col[b].cpu().numpy()].sum())
    S = u[:, :, None] + v[:, None, :] - (C.double() if dtype.is_floating_point else C.long())
    assert bool((S >= 0).all())
    assert not S.gather(2, col.long()[:, :, None]).any()
    fl = sh.check_duals_large(C, col, u, v, maximize=True)[3]
    assert not any(f & ~(0 if not dtype.is_floating_point else (TIGHT | SLACK)) for f in fl.cpu().tolist())
    assert any(sh.check_duals_large(C, col, u, v)[3].cpu().tolist())  # (not a certificate of the minimum)


# --------------------------------------------------------------------------- front end and the old sizes
@functools.lru_cache(maxsize=None)
def fixture_case(family, dtype, nr, nc):
    z, meta = load_npz_cases("lsap_large_cases.npz")
    m = [m for m in meta if (m["family"], m["dtype"], m["nr"], m["nc"]) == (family, dtype, nr, nc)][0]
    C = L.instance(family, dtype, nr, nc, 0)
    assert F.matrix_sha(C) == m["sha"]
    return C, z[f"col{m['i']}"].astype(np.int64)


@pytest.mark.parametrize("family,dtype,nr,nc", L.FRONT_END_CASES, ids=[c[0] for c in L.FRONT_END_CASES])
def test_linear_sum_assignment_large_at_the_reference_block_size(sh, family, dtype, nr, nc):
    """2000 x 2000, the reference's singles block: scipy's answer from the
    fixture, on the float64 route and on the exact integer route; tall input
    and the duals with it."""
    C, want = fixture_case(family, dtype, nr, nc)
    from santa_hip import lsap
    assert lsap.exact_int64_route(C) == (dtype == "int64")
    r, c = sh.linear_sum_assignment_large(C)
    assert r.dtype == np.int64 and c.dtype == np.int64
    assert np.array_equal(r, np.arange(nr)) and np.array_equal(c, want)
    r2, c2, u, v = sh.linear_sum_assignment_large(C, duals=True)
    assert np.array_equal(r2, r) and np.array_equal(c2, c)
    assert u.dtype == v.dtype == (np.int64 if dtype == "int64" else np.float64)
    if dtype == "int64":
        S = C - u[:, None] - v[None, :]
        assert (S >= 0).all() and not S[r, c].any() and int(u.sum() + v.sum()) == int(C[r, c].sum())
    T = np.ascontiguousarray(C[:, :1500])  # tall: 2000 x 1500
    r, c = sh.linear_sum_assignment_large(T)
    wr, wc = oracle.lsap(T)
    assert np.array_equal(r, wr) and np.array_equal(c, wc)
    with pytest.raises(ValueError, match="1024"):
        sh.linear_sum_assignment(C)


@pytest.mark.parametrize("dtype", ["int64", "int32", "float64", "float16"])
def test_up_to_1024_columns_the_large_entries_return_solve_batched_bits(sh, dtype):
    nr, nc = 300, 513
    if dtype in ("int64", "int32"):
        C = torch.from_numpy(np.stack([F.instance("i32_extremes", "int64", nr, nc, k) for k in range(3)]))
        C = C.to(getattr(torch, dtype)).cuda()
        flag_list = INT_FLAGS
    else:
        C = torch.from_numpy(np.stack([F.instance("decimal", "float64", nr, nc, k) for k in range(3)]))
        C = C.to(getattr(torch, dtype)).cuda()
        flag_list = (0, SH_FLAG_F64_MW, SH_FLAG_F64_SW)
    shapes = [(300, 513), (1, 513), (200, 200)]
    for flags in flag_list:
        for kw in ({}, {"shapes": shapes}, {"maximize": True}):
            a = sh.solve_batched(C, flags=flags, duals=True, **kw)
            b = sh.solve_batched_large(C, flags=flags, duals=True, **kw)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                                                          y.view(torch.int64) if y.dtype == torch.float64 else y)
            a0, b0 = sh.solve_batched(C, flags=flags, **kw), sh.solve_batched_large(C, flags=flags, **kw)
            assert torch.equal(a0[0], b0[0]) and torch.equal(a0[1].double().view(torch.int64),
                                                             b0[1].double().view(torch.int64))
            ca = sh.check_duals(C, a[0], a[2], a[3], **kw)
            cb = sh.check_duals_large(C, b[0], b[2], b[3], **kw)
            for x, y in zip(ca, cb):
                assert torch.equal(x.double().view(torch.int64), y.double().view(torch.int64))
    Ct = C.transpose(1, 2).contiguous()  # tall
    a, b = sh.solve_batched(Ct, duals=True), sh.solve_batched_large(Ct, duals=True)
    for x, y in zip(a, b):
        assert torch.equal(x.double().view(torch.int64), y.double().view(torch.int64))
