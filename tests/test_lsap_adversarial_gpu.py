"""GPU parity of the batched LSAP solvers on the structured and extreme-value
families of lsap_families.py: Machol-Wien instances (Dijkstras of nr / 2 steps,
an augmenting path of nr hops), values that put single steps of a solve
outside, inside and on the edges of the packed key's window, negative int32
values and both ends of its range, subnormals, a dtype's largest finite value,
float64 sums that overflow.  Columns are compared for equality with the CPU
oracle (and with scipy's fixture answers where the case is in
tests/golden/lsap_adversarial_cases.npz), integer costs for equality, float
costs against their rounding bound.

Measured on one MI355X: the 182 cases take 15 s together, the CPU oracle's
reference solves included.  The 1024-column Machol-Wien cases are the slowest:
3.2 s for mw_tenths (three float kernels), 1.8 s / 1.4 s for mw as int64 /
int32; every other case stays under 0.5 s."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_families as F  # noqa: E402
import oracle  # noqa: E402
from conftest import load_npz_cases  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_EXACT_ARGMIN = 2
SH_FLAG_F64_MW = 16384
SH_FLAG_F64_SW = 32768
INT_FLAGS = (0, SH_FLAG_EXACT_ARGMIN)
F64_FLAGS = (SH_FLAG_F64_SW, SH_FLAG_F64_MW, 0)


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


@functools.lru_cache(maxsize=None)
def fixture_cols():
    """(family, dtype, nr, nc) -> scipy's per-row columns (seed 0)."""
    z, meta = load_npz_cases("lsap_adversarial_cases.npz")
    return {(m["family"], m["dtype"], m["nr"], m["nc"]): z[f"col{m['i']}"].astype(np.int64) for m in meta}


def per_row(nr, row, col):
    """scipy's (row_ind, col_ind) as solve_batched's per-row columns (-1: none)."""
    want = -np.ones(nr, dtype=np.int64)
    want[np.asarray(row, dtype=np.int64)] = col
    return want


def oracle_cols(C):
    """Per-row columns [B, nr] of a [B, nr, nc] batch (int64: exact, else
    float64); -1 in every row of an infeasible instance."""
    cols = []
    for Cb in C:
        try:
            r, c = oracle.lsap(np.ascontiguousarray(Cb))
            cols.append(per_row(Cb.shape[0], r, c))
        except ValueError:
            cols.append(-np.ones(Cb.shape[0], dtype=np.int64))
    return np.stack(cols)


@functools.lru_cache(maxsize=None)
def batch(family, dtype, nr, nc, B):
    """(the batch, its oracle columns): instance k of a family is
    lsap_families.instance(.., k); instance 0 is the fixture's matrix.  The
    batch is an int64 / float64 numpy array or a CPU tensor of a narrow dtype."""
    inst = [F.instance(family, dtype, nr, nc, k) for k in range(B)]
    if dtype in F.NARROW:
        C = torch.stack(inst)
        ocol = oracle_cols(C.double().numpy())
    else:
        C = np.stack(inst)
        ocol = oracle_cols(C)
    fx = fixture_cols().get((family, dtype, nr, nc))
    if fx is not None:  # scipy itself, where the fixture has the case
        assert np.array_equal(ocol[0], fx), (family, dtype, nr, nc)
    return C, ocol


def bits(t):
    return t.view(torch.int64)


def check_cost_bound(C64, col, cost, nc):
    """|cost - exact sum| <= nc * 2^-53 * sum|chosen| for a fixed-order sum of
    nr <= nc terms, wherever that bound is finite (math.fsum raises
    OverflowError where the exact sum, or the sum of magnitudes, is not).
    Returns the number of instances checked."""
    checked = 0
    for b in range(C64.shape[0]):
        if (col[b] < 0).any():
            assert float(cost[b]) == 0.0, b
            continue
        chosen = C64[b, np.arange(C64.shape[1]), col[b]]
        try:
            exact = math.fsum(chosen.tolist())
            bound = nc * 2.0 ** -53 * math.fsum(np.abs(chosen).tolist())
        except OverflowError:
            continue
        if not math.isfinite(bound):
            continue
        assert abs(float(cost[b]) - exact) <= bound, (b, float(cost[b]), exact)
        checked += 1
    return checked


# --------------------------------------------------------------------------- integer solver
# every launch configuration, square and RECT: one wave (n <= 64), four waves
# x 1 (n <= 256), x 2 (n <= 512), x 4 columns per thread
INT_SHAPES = [(64, 64), (63, 64), (65, 65), (255, 256), (256, 256), (257, 257), (300, 513)]
INT_CASES = [(f, nr, nc, "int64") for f in F.INT_FAMILIES for nr, nc in INT_SHAPES]
INT_CASES += [(f, 1000, 1024, "int64") for f in ("mw", "two_scale43", "neg_cols", "window_edges")]
INT_CASES += [(f, nr, nc, "int32") for f in F.INT32_FAMILIES for nr, nc in INT_SHAPES]
# (mw_neg alone would not notice a load that lost the sign: 2^32 more in every
#  entry moves no decision.  i32_extremes mixes the signs, so it runs at 1024 too.)
INT_CASES += [(f, 1000, 1024, "int32") for f in ("mw", "i32_extremes")]


@pytest.mark.parametrize("family,nr,nc,dtype", INT_CASES, ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in INT_CASES])
def test_integer_families(sh, family, nr, nc, dtype):
    C, ocol = batch(family, "int64", nr, nc, 2 if nc == 1024 else 3)
    want = [int(C[b, np.arange(nr), ocol[b]].sum()) for b in range(C.shape[0])]
    Ct = torch.from_numpy(C).cuda()
    if dtype == "int32":
        Ct = Ct.to(torch.int32)
        assert torch.equal(Ct.cpu().long(), torch.from_numpy(C))  # (the family fits int32)
    for flags in INT_FLAGS:
        col, cost = sh.solve_batched(Ct, flags=flags)
        assert cost.dtype == torch.int64
        assert np.array_equal(col.cpu().numpy(), ocol), (family, nr, nc, dtype, flags)
        assert cost.cpu().tolist() == want, (family, nr, nc, dtype, flags)


@pytest.mark.parametrize("B,nr,nc", [(4096, 100, 128), (65536, 64, 129)], ids=["1x2-4096x100x128", "1x4-65536x64x129"])
def test_one_wave_large_batch_configs(sh, B, nr, nc):
    """One wave per instance with 2 (B >= 4096, nc <= 128) or 4 (B >= 65536,
    nc <= 256) columns per thread, on int32: mw_ties plus 0..3 of noise per
    entry, built on the device.  A few instances against the oracle, every
    instance against the same instances solved 1024 at a time (four waves).
    Then the whole batch 8 lower, which mixes the signs: a constant moves
    every path length of a Dijkstra alike and ends up in u, so scipy's
    decisions stay and the cost drops by 8 nr (a load that lost the sign
    would move the negative entries only)."""
    g = torch.Generator(device="cuda").manual_seed(9100 + nc)
    C = torch.randint(0, 4, (B, nr, nc), generator=g, dtype=torch.int32, device="cuda")
    C += torch.from_numpy(F.mw_ties(nr, nc)).to("cuda", torch.int32)
    col, cost = sh.solve_batched(C)
    Cm = C - 8
    assert bool((Cm[0] < 0).any()) and bool((Cm[0] > 0).any())
    colm, costm = sh.solve_batched(Cm)
    for b in (0, 1, 17, B - 1):
        for X, xcol, xcost in ((C, col, cost), (Cm, colm, costm)):
            Cb = X[b].cpu().numpy().astype(np.int64)
            _, oc = oracle.lsap(Cb)
            assert np.array_equal(xcol[b].cpu().numpy(), oc), (B, nr, nc, b)
            assert int(xcost[b]) == int(Cb[np.arange(nr), oc].sum()), (B, nr, nc, b)
    assert torch.equal(colm, col) and torch.equal(costm, cost - 8 * nr)
    for s in range(0, B, 1024):
        col4, cost4 = sh.solve_batched(C[s:s + 1024])
        assert torch.equal(col[s:s + 1024], col4) and torch.equal(cost[s:s + 1024], cost4), (B, nr, nc, s)


@pytest.mark.parametrize("B,nr,nc", [(4096, 100, 128), (65536, 64, 129)], ids=["1x2-4096x100x128", "1x4-65536x64x129"])
def test_one_wave_large_batch_window_families(sh, B, nr, nc):
    """The same two configurations on int64 with steps above, below and on the
    edges of the key's window (int32 cannot leave it): 24 host matrices, six
    seeds of four families, repeated over the batch; every instance against
    the oracle's answer for its matrix."""
    fams = ("window_edges", "neg_cols", "two_scale43", "i32_extremes")
    M = np.stack([F.make(f, "int64", nr, nc, seed) for f in fams for seed in range(6)])
    ocol = oracle_cols(M)
    ocost = np.array([int(M[m, np.arange(nr), ocol[m]].sum()) for m in range(len(M))], dtype=np.int64)
    idx = torch.arange(B, device="cuda") % len(M)
    C = torch.from_numpy(M).cuda()[idx]
    for flags in INT_FLAGS:
        col, cost = sh.solve_batched(C, flags=flags)
        assert torch.equal(col, torch.from_numpy(ocol.astype(np.int32)).cuda()[idx]), (B, nr, nc, flags)
        assert torch.equal(cost, torch.from_numpy(ocost).cuda()[idx]), (B, nr, nc, flags)


# --------------------------------------------------------------------------- float solvers
F64_SHAPES = [(64, 65), (130, 130), (100, 257), (257, 257), (300, 513)]
F64_CASES = [(f, nr, nc) for f in F.F64_FAMILIES for nr, nc in F64_SHAPES] + [("mw_tenths", 1000, 1024)]


@pytest.mark.parametrize("family,nr,nc", F64_CASES, ids=[f"{f}-{nr}x{nc}-float64" for f, nr, nc in F64_CASES])
def test_float64_families(sh, family, nr, nc):
    """One wave x 2 .. 16 columns per lane, four waves x 1, 2, 4 per thread and
    the default choice.  An instance the oracle finds infeasible (sums that
    overflow to +inf everywhere) gives -1 in every row and cost 0."""
    C, ocol = batch(family, "float64", nr, nc, 2 if nc == 1024 else 3)
    Cd = torch.from_numpy(C).cuda()
    costs = []
    for flags in F64_FLAGS:
        col, cost = sh.solve_batched(Cd, flags=flags)
        assert np.array_equal(col.cpu().numpy(), ocol), (family, nr, nc, flags)
        costs.append(cost)
    assert torch.equal(bits(costs[0]), bits(costs[1])) and torch.equal(bits(costs[0]), bits(costs[2]))
    checked = check_cost_bound(C, ocol, costs[0].cpu().numpy(), nc)
    if family not in ("huge", "max_overflow", "neg_max"):  # (finite sums: every instance is checked)
        assert checked == C.shape[0]


NARROW_SHAPES = [(64, 65), (130, 130), (300, 513)]
NARROW_CASES = [(f, nr, nc, d) for d in sorted(F.NARROW) for f in F.NARROW_NAMES for nr, nc in NARROW_SHAPES]


@pytest.mark.parametrize("family,nr,nc,dtype", NARROW_CASES,
                         ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in NARROW_CASES])
def test_narrow_families(sh, family, nr, nc, dtype):
    """Subnormals, +-finfo.max and the tie-heavy long paths read at their own
    width: the oracle's columns on the widened matrix, and col and cost bit
    for bit those of C.double(), whichever kernel runs."""
    Ct, ocol = batch(family, dtype, nr, nc, 3)
    assert Ct.dtype == F.NARROW[dtype]
    Cd = Ct.cuda()
    C64 = Cd.double()
    assert torch.equal(C64.cpu(), Ct.double())  # (the device's widening of the tensor is the host's)
    costs = []
    for flags in F64_FLAGS:
        col, cost = sh.solve_batched(Cd, flags=flags)
        col64, cost64 = sh.solve_batched(C64, flags=flags)
        assert cost.dtype == torch.float64
        assert np.array_equal(col.cpu().numpy(), ocol), (family, nr, nc, dtype, flags)
        assert torch.equal(col, col64) and torch.equal(bits(cost), bits(cost64)), (family, nr, nc, dtype, flags)
        costs.append(cost)
    assert torch.equal(bits(costs[0]), bits(costs[1])) and torch.equal(bits(costs[0]), bits(costs[2]))
    assert check_cost_bound(Ct.double().numpy(), ocol, costs[0].cpu().numpy(), nc) == 3


# --------------------------------------------------------------------------- the front end
FRONT = [("window_edges", "int64", 255, 256, np.int64),    # the exact int64 route
         ("window_edges", "int64", 1000, 1024, np.int64),  # past its bound: the float64 replay
         ("i32_extremes", "int64", 300, 513, np.int32),
         ("mw_tenths", "float64", 257, 257, np.float64)]


@pytest.mark.parametrize("family,dtype,nr,nc,np_dtype", FRONT,
                         ids=[f"{f}-{nr}x{nc}-{np.dtype(t).name}" for f, _, nr, nc, t in FRONT])
def test_linear_sum_assignment_front_end(sh, family, dtype, nr, nc, np_dtype):
    C = F.make(family, dtype, nr, nc)
    A = C.astype(np_dtype)
    assert np.array_equal(A, C)
    r, c = sh.linear_sum_assignment(A)
    assert np.array_equal(r, np.arange(nr)) and np.array_equal(c, fixture_cols()[family, dtype, nr, nc])
