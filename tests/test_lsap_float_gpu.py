"""GPU parity of the floating-point batched LSAP: float32 / float16 / bfloat16
costs read at their own width, and the one-wave and four-wave float64 replay
kernels (SH_FLAG_F64_SW / SH_FLAG_F64_MW), against the CPU oracle on the
widened float64 matrix.  Columns are compared for equality; a narrow dtype's
col and cost are bit-identical to those of the same tensor after .double();
the cost, a fixed-order sum, is within its rounding bound of the exact sum."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_F64_MW = 16384
SH_FLAG_F64_SW = 32768
DESIGNS = (SH_FLAG_F64_SW, SH_FLAG_F64_MW)
ALL_FLAGS = (SH_FLAG_F64_SW, SH_FLAG_F64_MW, 0)
NARROW = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


def per_row(nr, row, col):
    """scipy's (row_ind, col_ind) as solve_batched's per-row columns (-1: none)."""
    want = -np.ones(nr, dtype=np.int64)
    want[np.asarray(row, dtype=np.int64)] = col
    return want


def oracle_cols(C):
    """Per-row columns [B, nr] of a float64 [B, nr, nc] batch; -1 in every row
    of an infeasible instance."""
    cols = []
    for Cb in C:
        try:
            r, c = oracle.lsap(np.ascontiguousarray(Cb))
            cols.append(per_row(Cb.shape[0], r, c))
        except ValueError:
            cols.append(-np.ones(Cb.shape[0], dtype=np.int64))
    return np.stack(cols)


def widened(Ct):
    """The float64 image of a tensor of any float dtype, as numpy (exact)."""
    return Ct.double().numpy()


@functools.lru_cache(maxsize=None)
def values(kind, nr, nc, dtype, B=3):
    """(CPU tensor of `dtype`, its oracle columns).  kind 'ties': randint(0, 3)
    * 0.5, exact in every float dtype; 'wide': randn * 100 cast to the dtype."""
    rng = np.random.default_rng([11000, kind == "ties", nr, nc])
    if kind == "ties":
        C = rng.integers(0, 3, size=(B, nr, nc)) * 0.5
    else:
        C = rng.standard_normal((B, nr, nc)) * 100
    Ct = torch.from_numpy(C).to(dtype)
    return Ct, oracle_cols(widened(Ct))


def check_cost_bound(C64, col, cost, nc):
    for b in range(C64.shape[0]):
        nr = C64.shape[1]
        chosen = C64[b, np.arange(nr), col[b]]
        exact = math.fsum(chosen.tolist())
        assert abs(float(cost[b]) - exact) <= nc * 2.0 ** -53 * math.fsum(np.abs(chosen).tolist()), b


# --------------------------------------------------------------------------- 1: fails without the feature
def test_float32_is_accepted(sh):
    rng = np.random.default_rng(1)
    C = (rng.standard_normal((3, 63, 65)) * 100).astype(np.float32)
    col, cost = sh.solve_batched(torch.from_numpy(C).cuda())
    assert col.dtype == torch.int32 and cost.dtype == torch.float64
    assert np.array_equal(col.cpu().numpy(), oracle_cols(C.astype(np.float64)))


# --------------------------------------------------------------------------- 2: dtype parity
@pytest.mark.parametrize("nr,nc", [(1, 64), (63, 65), (100, 257), (300, 513), (500, 1024)])
@pytest.mark.parametrize("dtype", sorted(NARROW))
def test_narrow_dtype_parity(sh, dtype, nr, nc):
    for kind in ("ties", "wide"):
        Ct, ocol = values(kind, nr, nc, NARROW[dtype])
        assert Ct.dtype == NARROW[dtype]
        Cd = Ct.cuda()
        col, cost = sh.solve_batched(Cd)
        col64, cost64 = sh.solve_batched(Cd.double())
        assert cost.dtype == torch.float64
        assert np.array_equal(col.cpu().numpy(), ocol), (dtype, nr, nc, kind)
        assert torch.equal(col, col64) and torch.equal(cost, cost64), (dtype, nr, nc, kind)
        check_cost_bound(widened(Ct), col.cpu().numpy(), cost.cpu().numpy(), nc)


# --------------------------------------------------------------------------- 3: both designs, every configuration's edges
EDGES = [(1, 65), (64, 65), (255, 256), (100, 257), (257, 512), (300, 513), (1000, 1024), (1, 1024)]


@pytest.mark.parametrize("nr,nc", EDGES)
def test_both_designs_at_configuration_edges(sh, nr, nc):
    """Four waves x 1, 2, 4 columns per thread (nc <= 256, 512, 1024) and one
    wave x 2 .. 16 columns per lane, few rows and nearly square."""
    for dt in (torch.float64, torch.float32):
        for kind in ("ties", "wide"):
            Ct, ocol = values(kind, nr, nc, dt)
            Cd = Ct.cuda()
            costs = []
            for flags in ALL_FLAGS:
                col, cost = sh.solve_batched(Cd, flags=flags)
                assert np.array_equal(col.cpu().numpy(), ocol), (nr, nc, dt, kind, flags)
                costs.append(cost)
            assert torch.equal(costs[0], costs[1]) and torch.equal(costs[0], costs[2]), (nr, nc, dt, kind)
            check_cost_bound(widened(Ct), ocol, costs[0].cpu().numpy(), nc)


# --------------------------------------------------------------------------- 4: signed zeros
@pytest.mark.parametrize("nr,nc", [(64, 65), (200, 257)])
def test_signed_zeros(sh, nr, nc):
    """-0.0 and +0.0 tie (scipy compares values); a minimum taken on the bit
    patterns would separate them."""
    rng = np.random.default_rng(77 + nr)
    C = np.array([-0.0, 0.0, -0.5, 0.5])[rng.integers(0, 4, size=(3, nr, nc))]
    assert np.signbit(C[C == 0]).any() and not np.signbit(C[C == 0]).all()
    ocol = oracle_cols(C)
    for dt in (torch.float64, torch.float16):
        Cd = torch.from_numpy(C).to(dt).cuda()
        assert np.array_equal(np.signbit(widened(Cd.cpu())), np.signbit(C))
        for flags in ALL_FLAGS:
            col, _ = sh.solve_batched(Cd, flags=flags)
            assert np.array_equal(col.cpu().numpy(), ocol), (nr, nc, dt, flags)


# --------------------------------------------------------------------------- 5: +inf
def _inf_square_batch(n, k, rng):
    """[feasible, infeasible, feasible] n x n: 30 % +inf over a finite diagonal
    band; the infeasible one has k + 1 rows finite only in the same k columns."""
    C = rng.integers(0, 1000, size=(3, n, n)).astype(np.float64)
    i, j = np.indices((n, n))
    band = np.abs(i - j) <= 2
    for b in range(3):
        C[b][(rng.random((n, n)) < 0.3) & ~band] = np.inf
    cols = rng.choice(n, size=k, replace=False)
    rows = rng.choice(n, size=k + 1, replace=False)
    blocked = np.ones(n, dtype=bool)
    blocked[cols] = False
    for r in rows:
        C[1, r, blocked] = np.inf
    return C


def _inf_wide_batch(rng, nr=40, nc=130):
    """[feasible, dry] nr x nc: the dry instance has its finite entries
    confined to nr - 1 columns, so a Dijkstra runs dry with columns left."""
    C = rng.integers(0, 1000, size=(2, nr, nc)).astype(np.float64)
    C[0][rng.random((nr, nc)) < 0.3] = np.inf
    C[0, np.arange(nr), np.arange(nr)] = 5.0
    keep = rng.choice(nc, size=nr - 1, replace=False)
    dead = np.ones(nc, dtype=bool)
    dead[keep] = False
    C[1][:, dead] = np.inf
    return C


@pytest.mark.parametrize("case", ["square", "wide"])
def test_inf_entries_and_infeasible_instances(sh, case):
    rng = np.random.default_rng(505)
    C = _inf_square_batch(130, 17, rng) if case == "square" else _inf_wide_batch(rng)
    ocol = oracle_cols(C)
    infeasible = [1]
    for b in range(C.shape[0]):
        assert (ocol[b] == -1).all() == (b in infeasible), b
    for dt in (torch.float64, torch.float32):
        Cd = torch.from_numpy(C).to(dt).cuda()  # (integers below 1000 and +inf: exact in float32)
        for flags in ALL_FLAGS:
            col, cost = sh.solve_batched(Cd, flags=flags)
            assert np.array_equal(col.cpu().numpy(), ocol), (case, dt, flags)
            assert float(cost[1]) == 0.0
            feas = [b for b in range(C.shape[0]) if b not in infeasible]
            for b in feas:
                assert float(cost[b]) == float(C[b, np.arange(C.shape[1]), ocol[b]].sum()), (case, b)


# --------------------------------------------------------------------------- 6: ragged, tall, maximize in a narrow dtype
RAGGED = [(0, 0), (1, 1), (64, 65), (70, 140), (17, 65), (3, 129), (64, 64), (70, 70)]


@pytest.mark.parametrize("padding", ["nan", "attractive"])
def test_ragged_float16(sh, padding):
    """One padded [8, 70, 140] float16 batch.  The padding holds NaN, or a
    value more attractive than any live entry: a solver that read it would
    fail or choose it."""
    rng = np.random.default_rng(61)
    NR, NC = 70, 140
    P = np.full((len(RAGGED), NR, NC), np.nan if padding == "nan" else -4096.0)
    for b, (nr, nc) in enumerate(RAGGED):
        P[b, :nr, :nc] = rng.integers(0, 3, size=(nr, nc)) * 0.5 if b % 2 else rng.integers(0, 2048, size=(nr, nc))
    Pt = torch.from_numpy(P).to(torch.float16)
    assert np.array_equal(widened(Pt), P, equal_nan=True)  # (exact in float16)
    Pd = Pt.cuda()
    want = -np.ones((len(RAGGED), NR), dtype=np.int64)
    wcost = np.zeros(len(RAGGED))
    for b, (nr, nc) in enumerate(RAGGED):
        if nr:
            want[b, :nr] = oracle_cols(P[b:b + 1, :nr, :nc])[0]
            wcost[b] = P[b, np.arange(nr), want[b, :nr]].sum()  # (integers and halves: exact sums)
    for flags in ALL_FLAGS:
        col, cost = sh.solve_batched(Pd, shapes=np.array(RAGGED), flags=flags)
        assert np.array_equal(col.cpu().numpy(), want), (padding, flags)
        assert np.array_equal(cost.cpu().numpy(), wcost), (padding, flags)


def test_tall_bfloat16(sh):
    """[3, 300, 100]: solved as the transpose and inverted on the device; the
    -1 rows are exactly the rows scipy leaves out."""
    rng = np.random.default_rng(62)
    Ct = torch.from_numpy(rng.standard_normal((3, 300, 100)) * 100).to(torch.bfloat16)
    ocol = oracle_cols(widened(Ct))
    assert ((ocol < 0).sum(axis=1) == 200).all()
    for flags in ALL_FLAGS:
        col, cost = sh.solve_batched(Ct.cuda(), flags=flags)
        assert tuple(col.shape) == (3, 300)
        assert np.array_equal(col.cpu().numpy(), ocol), flags
        col64, cost64 = sh.solve_batched(Ct.cuda().double(), flags=flags)
        assert torch.equal(col, col64) and torch.equal(cost, cost64)


def test_maximize_float32(sh):
    rng = np.random.default_rng(63)
    Ct = torch.from_numpy(rng.standard_normal((3, 100, 257)) * 100).to(torch.float32)
    C64 = widened(Ct)
    ocol = oracle_cols(-C64)
    for flags in ALL_FLAGS:
        col, cost = sh.solve_batched(Ct.cuda(), flags=flags, maximize=True)
        assert np.array_equal(col.cpu().numpy(), ocol), flags
        check_cost_bound(C64, ocol, cost.cpu().numpy(), 257)  # (the maximum itself, not its negation)


def test_empty_cases_in_a_narrow_dtype(sh):
    for shape in ((0, 4, 5), (2, 0, 5), (2, 4, 0)):
        col, cost = sh.solve_batched(torch.zeros(shape, dtype=torch.bfloat16, device="cuda"))
        assert tuple(col.shape) == shape[:2] and (col == -1).all()
        assert cost.dtype == torch.float64 and tuple(cost.shape) == shape[:1] and (cost == 0).all()


# --------------------------------------------------------------------------- 7: a large batch
def test_large_batch_float32(sh):
    """4096 instances of 40 x 100, tie-heavy: every instance against the oracle."""
    B, nr, nc = 4096, 40, 100
    rng = np.random.default_rng(64)
    C = (rng.integers(0, 3, size=(B, nr, nc)) * 0.5).astype(np.float32)
    col, cost = sh.solve_batched(torch.from_numpy(C).cuda())
    col, cost = col.cpu().numpy(), cost.cpu().numpy()
    C64 = C.astype(np.float64)
    rows = np.arange(nr)
    for b in range(B):
        _, oc = oracle.lsap(C64[b])
        assert np.array_equal(col[b], oc), b
        assert cost[b] == C64[b, rows, oc].sum(), b  # (halves: exact sums)
