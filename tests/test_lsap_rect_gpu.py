"""GPU parity of the rectangular / ragged batched LSAP: the HIP solvers
(through the C-ABI and the Python front end) against scipy's fixture answers
and the CPU oracle.  Every result is an exact integer: equality throughout
(the float64 cost, a fixed-order sum, within its rounding bound)."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from conftest import load_npz_cases  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_EXACT_ARGMIN = 2


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


@pytest.fixture(scope="module")
def rect_cases():
    return load_npz_cases("lsap_rect_cases.npz")


def per_row(nr, row, col):
    """scipy's (row_ind, col_ind) as solve_batched's per-row columns (-1: none)."""
    want = -np.ones(nr, dtype=np.int64)
    want[np.asarray(row, dtype=np.int64)] = col
    return want


def oracle_batch(C):
    """(per-row columns [B, nr], cost [B] as Python numbers) of a [B, nr, nc] batch."""
    cols, costs = [], []
    for Cb in C:
        r, c = oracle.lsap(Cb)
        cols.append(per_row(Cb.shape[0], r, c))
        costs.append(Cb[r, c].sum().item() if Cb.dtype == np.int64 else math.fsum(Cb[r, c].tolist()))
    return np.stack(cols), costs


# --------------------------------------------------------------------------- golden
def test_rect_golden_linear_sum_assignment(sh, rect_cases):
    z, meta = rect_cases
    for m in meta:
        C = z[f"C{m['i']}"]
        C = C.astype(np.int64) if m["kind"] == "int" else C
        if not m["feasible"]:
            with pytest.raises(ValueError, match="infeasible"):
                sh.linear_sum_assignment(C, maximize=m["maximize"])
            continue
        r, c = sh.linear_sum_assignment(C, maximize=m["maximize"])
        assert r.dtype == np.int64 and c.dtype == np.int64
        assert np.array_equal(r, z[f"row{m['i']}"]) and np.array_equal(c, z[f"col{m['i']}"]), m


def test_rect_golden_solve_batched(sh, rect_cases):
    """Every fixture case as a batch of one: integer cases as int64, int32 and
    float64, float cases as float64; tall cases give -1 in the rows scipy
    leaves out, infeasible ones -1 everywhere."""
    z, meta = rect_cases
    for m in meta:
        C = z[f"C{m['i']}"]
        nr = m["nr"]
        want = per_row(nr, z[f"row{m['i']}"], z[f"col{m['i']}"]) if m["feasible"] else -np.ones(nr)
        dts = (torch.int64, torch.int32, torch.float64) if m["kind"] == "int" else (torch.float64,)
        for dt in dts:
            Ct = torch.from_numpy(C.astype(np.int64) if m["kind"] == "int" else C)[None].to("cuda", dt)
            col, cost = sh.solve_batched(Ct, maximize=m["maximize"])
            assert col.dtype == torch.int32 and tuple(col.shape) == (1, nr)
            assert np.array_equal(col[0].cpu().numpy(), want), (m, dt)
            if m["feasible"] and dt != torch.float64:
                assert int(cost[0]) == int(m["cost"]), (m, dt)
            elif m["feasible"]:
                # two sums of at most n = max(nr, nc) terms in different orders (the
                # fixture's is numpy's): each within n * 2^-53 * sum|chosen| of the exact sum
                sel = np.abs(C[z[f"row{m['i']}"], z[f"col{m['i']}"]].astype(np.float64))
                assert abs(float(cost[0]) - m["cost"]) <= 2 * max(m["nr"], m["nc"]) * 2.0 ** -53 * sel.sum(), m


# --------------------------------------------------------------------------- boundary shapes
BOUNDARY = [(1, 64), (63, 64), (1, 65), (64, 65), (5, 256), (255, 256), (100, 257), (257, 512), (300, 513),
            (1000, 1024), (1, 1024)]


@pytest.mark.parametrize("nr,nc", BOUNDARY)
def test_rect_boundary_shapes_vs_oracle(sh, nr, nc):
    """Every launch configuration's edges (1 wave; 4 waves x 1, 2, 4 columns),
    few rows and nearly square, heavy ties and wide values; the exact two-pass
    argmin must agree with the packed-key one."""
    rng = np.random.default_rng(7000 + 1031 * nr + nc)
    for mod in (3, 1 << 16):
        C = rng.integers(0, mod, size=(3, nr, nc), dtype=np.int64)
        ocol, ocost = oracle_batch(C)
        Ct = torch.from_numpy(C).cuda()
        for flags in (0, SH_FLAG_EXACT_ARGMIN):
            col, cost = sh.solve_batched(Ct, flags=flags)
            assert np.array_equal(col.cpu().numpy(), ocol), (nr, nc, mod, flags)
            assert cost.cpu().tolist() == ocost, (nr, nc, mod, flags)


@pytest.mark.parametrize("nr,nc", [(63, 65), (100, 257), (500, 1024)])
def test_rect_float64_vs_oracle(sh, nr, nc):
    """The one-wave float64 replay (K = 2, 8, 16 columns per lane) on
    tie-heavy values.  The cost is a fixed-order sum of nr <= nc terms: it may
    differ from the correctly rounded sum by at most nc * 2^-53 * sum|chosen|."""
    rng = np.random.default_rng(9000 + nr)
    C = rng.integers(0, 3, size=(3, nr, nc)) * 0.5
    ocol, ocost = oracle_batch(C)
    col, cost = sh.solve_batched(torch.from_numpy(C).cuda())
    col = col.cpu().numpy()
    assert np.array_equal(col, ocol)
    for b in range(3):
        chosen = C[b, np.arange(nr), col[b]]
        exact = math.fsum(chosen.tolist())
        assert abs(float(cost[b]) - exact) <= nc * 2.0 ** -53 * math.fsum(np.abs(chosen).tolist()), (b, nr, nc)


# --------------------------------------------------------------------------- one-wave large-batch configs
@pytest.mark.parametrize("nr,nc,B", [(40, 100, 4096), (100, 128, 8192), (8, 200, 65536)])
def test_rect_large_batch_configs_vs_oracle(sh, nr, nc, B):
    """Large batches run one wave per instance with 2 or 4 columns per thread:
    instances of the device-generated stream equal the oracle on the first nr
    rows of the host mirror's nc x nc matrix."""
    from santa_hip.sampler import hash_matrix
    col, cost = sh.solve_hash(5, 1 << 16, nc, B, device=0, nr=nr)
    assert tuple(col.shape) == (B, nr)
    col, cost = col.cpu().numpy(), cost.cpu().numpy()
    for b in (0, 1, B - 1):
        C = hash_matrix(5, b, nc, 1 << 16).astype(np.int64)[:nr]
        _, oc = oracle.lsap(C)
        assert np.array_equal(col[b], oc), (nr, nc, B, b)
        assert int(cost[b]) == int(C[np.arange(nr), oc].sum()), (nr, nc, B, b)


# --------------------------------------------------------------------------- ragged
RAGGED = [(0, 0), (1, 1), (64, 130), (64, 64), (17, 65), (3, 129)]


@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_ragged_batch_vs_oracle(sh, dtype):
    """One padded [6, 64, 130] batch of six shapes.  The padding holds a value
    at least as attractive as any live entry (int64) or NaN (float64): a
    solver that read it would choose it or fail."""
    rng = np.random.default_rng(31)
    NR, NC = 64, 130
    if dtype == "int64":
        P = np.full((len(RAGGED), NR, NC), -(2 ** 40), dtype=np.int64)
    else:
        P = np.full((len(RAGGED), NR, NC), np.nan)
    for b, (nr, nc) in enumerate(RAGGED):
        live = rng.integers(0, 3 if b % 2 else 1 << 16, size=(nr, nc))
        P[b, :nr, :nc] = live if dtype == "int64" else live * 0.5
    Pt = torch.from_numpy(P).cuda()
    for shapes in (np.array(RAGGED, dtype=np.int64), torch.tensor(RAGGED, dtype=torch.int32, device="cuda")):
        col, cost = sh.solve_batched(Pt, shapes=shapes)
        col = col.cpu().numpy()
        assert col.shape == (len(RAGGED), NR)
        for b, (nr, nc) in enumerate(RAGGED):
            assert (col[b, nr:] == -1).all(), b
            if nr == 0:
                assert float(cost[b]) == 0
                continue
            live = np.ascontiguousarray(P[b, :nr, :nc])
            _, oc = oracle.lsap(live)
            assert np.array_equal(col[b, :nr], oc), (b, nr, nc)
            assert float(cost[b]) == float(live[np.arange(nr), oc].sum()), b  # (halves: exact sums)


def test_ragged_rejects_tall_shapes_before_launch(sh):
    C = torch.zeros((2, 8, 8), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="transpose"):
        sh.solve_batched(C, shapes=[[3, 4], [5, 3]])
    with pytest.raises(ValueError, match="outside"):
        sh.solve_batched(C, shapes=[[3, 4], [9, 9]])
    with pytest.raises(ValueError, match="transpose"):  # a tall padded batch cannot be ragged
        sh.solve_batched(torch.zeros((2, 9, 8), dtype=torch.int64, device="cuda"), shapes=[[3, 4], [2, 3]])


def test_kernel_refuses_bad_shapes(sh):
    """The C-ABI's own guard (the front end never lets these through): an
    instance whose shape is outside 0 <= nr_b <= nc_b <= nc, nr_b <= nr gets
    col = -1 and cost 0, its neighbours are solved."""
    from santa_hip import _lib
    rng = np.random.default_rng(5)
    NR, NC = 8, 12
    shapes = [(8, 12), (5, 3), (-1, 4), (2, 13), (9, 12), (0, 0), (4, 4)]
    C = rng.integers(0, 50, size=(len(shapes), NR, NC), dtype=np.int64)
    for dt, entry in ((torch.int64, "lsap_solve_batched_rect_i64"), (torch.float64, "lsap_solve_batched_rect_f64")):
        Ct = torch.from_numpy(C).to("cuda", dt)
        st = torch.tensor(shapes, dtype=torch.int32, device="cuda")
        col = torch.full((len(shapes), NR), 77, dtype=torch.int32, device="cuda")
        cost = torch.full((len(shapes),), 77, dtype=dt, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = getattr(_lib.lib(), entry)(p(Ct), NR, NC, len(shapes), p(st), p(col), p(cost), 1, None)
        assert rc == 0
        torch.cuda.synchronize()
        col, cost = col.cpu().numpy(), cost.cpu().numpy()
        for b, (nr, nc) in enumerate(shapes):
            if b in (0, 6):
                _, oc = oracle.lsap(np.ascontiguousarray(C[b, :nr, :nc]))
                assert np.array_equal(col[b, :nr], oc) and (col[b, nr:] == -1).all()
                assert cost[b] == C[b, np.arange(nr), oc].sum()
            else:
                assert (col[b] == -1).all() and cost[b] == 0, (b, nr, nc)


# --------------------------------------------------------------------------- tall, maximize, square
def test_tall_batch_vs_oracle(sh):
    """[3, 130, 64]: solved as the transpose and inverted on the device; the
    -1 rows are exactly the rows scipy leaves out."""
    rng = np.random.default_rng(41)
    for mod in (3, 1 << 16):
        C = rng.integers(0, mod, size=(3, 130, 64), dtype=np.int64)
        ocol, ocost = oracle_batch(C)
        assert ((ocol < 0).sum(axis=1) == 130 - 64).all()
        col, cost = sh.solve_batched(torch.from_numpy(C).cuda())
        assert tuple(col.shape) == (3, 130)
        assert np.array_equal(col.cpu().numpy(), ocol), mod
        assert cost.cpu().tolist() == ocost
    Cf = rng.integers(0, 3, size=(3, 130, 64)) * 0.5
    col, _ = sh.solve_batched(torch.from_numpy(Cf).cuda())
    assert np.array_equal(col.cpu().numpy(), oracle_batch(Cf)[0])


def test_maximize_fixture_cases(sh, rect_cases):
    z, meta = rect_cases
    ms = [m for m in meta if m["maximize"]]
    assert {m["nr"] > m["nc"] for m in ms} == {False, True}  # one wide, one tall
    for m in ms:
        C = z[f"C{m['i']}"]
        C = C.astype(np.int64) if m["kind"] == "int" else C
        r, c = sh.linear_sum_assignment(C, maximize=True)
        assert np.array_equal(r, z[f"row{m['i']}"]) and np.array_equal(c, z[f"col{m['i']}"]), m
        col, cost = sh.solve_batched(torch.from_numpy(C)[None].cuda(), maximize=True)
        assert np.array_equal(col[0].cpu().numpy(), per_row(m["nr"], r, c))
        assert float(cost[0]) == m["cost"]  # (the maximum itself, not its negation)


@pytest.mark.parametrize("dt", [torch.int64, torch.int32, torch.float64])
def test_square_batch_unchanged(sh, dt):
    """A square batch: solve_batched (the rect entry with nr == nc and no
    shapes), the ragged path with full shapes and the square C-ABI entry give
    the same col and cost -- and the oracle's."""
    from santa_hip import _lib
    rng = np.random.default_rng(51)
    B, n = 4, 96
    C = rng.integers(0, 50, size=(B, n, n), dtype=np.int64)
    Ct = torch.from_numpy(C).to("cuda", dt)
    col, cost = sh.solve_batched(Ct)
    ocol, ocost = oracle.lsap_i64_batched(C)
    assert np.array_equal(col.cpu().numpy(), ocol) and cost.cpu().tolist() == ocost.tolist()
    col2, cost2 = sh.solve_batched(Ct, shapes=[[n, n]] * B)
    assert torch.equal(col, col2) and torch.equal(cost, cost2)
    entry = {torch.int64: "lsap_solve_batched_i64", torch.int32: "lsap_solve_batched_i32",
             torch.float64: "lsap_solve_batched_f64"}[dt]
    col3, cost3 = torch.empty_like(col), torch.empty_like(cost)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert getattr(_lib.lib(), entry)(p(Ct), n, B, p(col3), p(cost3), 1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(col, col3) and torch.equal(cost, cost3)
