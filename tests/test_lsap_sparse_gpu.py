"""GPU tests of the batched LSAP on sparse (CSR) costs: solve_batched_sparse
and linear_sum_assignment_sparse (the lsap_solve_csr_ entries).

The contract is one sentence -- a sparse instance is solved exactly as the
dense float solver solves its densification -- so every case of
lsap_sparse_families is compared, for each kernel the flags select, with the
CPU oracle (col), with the CPU replay of scipy's loop (u, v, bit for bit) and
with solve_batched_large on the densified tensor (cost, bit for bit: existing
code, not code under test).  The expectations are computed once per case
(lsap_sparse_families.expected) and pinned on the CPU by test_lsap_sparse_cpu."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_sparse_families as S  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_F64_MW = 16384
SH_FLAG_F64_SW = 32768
CASES = [(f, nr, nc, fl) for f, nr, nc in S.cases() for fl in (0, SH_FLAG_F64_MW, SH_FLAG_F64_SW)
         if not (fl == SH_FLAG_F64_SW and nc > 1024)]


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("solve_batched_sparse", "linear_sum_assignment_sparse", "densify"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def same_bits(a, b):
    """float64 arrays equal bit for bit, any NaN matching any NaN."""
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    b = np.ascontiguousarray(b.cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def device_csr(b, dtype=torch.float64):
    return (torch.from_numpy(b.indptr).cuda(), torch.from_numpy(b.indices).cuda(),
            torch.from_numpy(b.data).to(dtype).cuda())


def check_cost_bound(dense, col, cost, nc):
    """test_lsap_large_gpu.check_cost_bound on the live rows of each instance:
    |cost - exact sum| <= nc * 2^-53 * sum|chosen| for a fixed-order sum of
    nr <= nc terms; cost 0 where no assignment exists."""
    for k, D in enumerate(dense):
        live = col[k, :D.shape[0]]
        if D.shape[0] == 0 or (live < 0).any():
            assert float(cost[k]) == 0.0, k
            continue
        chosen = D[np.arange(D.shape[0]), live]
        exact = math.fsum(chosen.tolist())
        bound = nc * 2.0 ** -53 * math.fsum(np.abs(chosen).tolist())
        print(f"cost[{k}] = {float(cost[k])!r}, exact {exact!r}, bound {bound!r}")
        assert abs(float(cost[k]) - exact) <= bound, (k, float(cost[k]), exact)


@pytest.mark.parametrize("family,nr,nc,flags", CASES)
def test_sparse_solve_is_the_dense_solve_of_the_densification(sh, family, nr, nc, flags):
    b = S.batch(family, nr, nc)
    B = len(b.dense)
    wcol, wu, wv = S.expected(family, nr, nc)
    shapes = np.array(b.corners, dtype=np.int32) if b.corners else None
    crow, idx, val = device_csr(b)
    col, cost, u, v = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), flags=flags, shapes=shapes,
                                              duals=True)
    assert col.dtype == torch.int32 and tuple(col.shape) == (B, nr)
    assert cost.dtype == u.dtype == v.dtype == torch.float64
    col_h = col.cpu().numpy().astype(np.int64)
    assert np.array_equal(col_h, wcol)
    for k in range(B):  # (what the expectation holds, said once more in the issue's words)
        r, c = b.dense[k].shape
        if not b.feasible[k]:
            assert (col_h[k] == -1).all() and float(cost[k]) == 0.0
        if r == 0:  # an empty shape: zero duals in every slot
            assert not u[k].any() and not v[k].any()
        elif not b.feasible[k]:
            assert np.isnan(u[k, :r].cpu().numpy()).all() and np.isnan(v[k, :c].cpu().numpy()).all()
        assert (col_h[k, r:] == -1).all() and not u[k, r:].any() and not v[k, c:].any()
    assert same_bits(u, wu), "u differs from the replay of scipy's run"
    assert same_bits(v, wv), "v differs from the replay of scipy's run"
    # cost: the dense kernels' bits on the densified tensor, and within the rounding bound of the exact sum
    D = torch.from_numpy(S.padded_dense(b, nr, nc)).cuda()
    dcol, dcost = sh.solve_batched_large(D, flags=flags, shapes=shapes)
    assert torch.equal(dcol, col) and same_bits(cost, dcost)
    check_cost_bound(b.dense, col_h, cost.cpu().numpy(), nc)
    # float32 storage gives the bits of float64 storage (the values are exact in float32)
    col32, cost32, u32, v32 = sh.solve_batched_sparse(crow, idx, val.float(), shape=(B, nr, nc), flags=flags,
                                                      shapes=shapes, duals=True)
    assert torch.equal(col32, col) and same_bits(cost32, cost) and same_bits(u32, u) and same_bits(v32, v)
    # duals=False gives the bits of duals=True
    col0, cost0 = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), flags=flags, shapes=shapes)
    assert torch.equal(col0, col) and same_bits(cost0, cost)
    colnc, none = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), flags=flags, shapes=shapes,
                                          with_cost=False)
    assert none is None and torch.equal(colnc, col)


@pytest.mark.parametrize("family,nr,nc", [("band_5pct", 64, 64), ("explicit_zero", 100, 257),
                                          ("band_40pct", 40, 2049), ("hall", 63, 65)])
def test_maximize_is_the_solve_of_the_negated_values(sh, family, nr, nc):
    b = S.batch(family, nr, nc)
    B = len(b.dense)
    crow, idx, val = device_csr(b)
    col, cost, u, v = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), maximize=True, duals=True)
    ncol, ncost, nu, nv = sh.solve_batched_sparse(crow, idx, -val, shape=(B, nr, nc), duals=True)
    assert torch.equal(col, ncol) and same_bits(cost, -ncost) and same_bits(u, -nu) and same_bits(v, -nv)
    assert bool((col >= 0).all()) == (family != "hall")
    if family != "hall":  # and it is a maximum: the oracle's, on the negated densification
        import oracle
        for k in range(B):
            assert np.array_equal(col[k].cpu().numpy(), oracle.lsap(np.where(np.isinf(b.dense[k]), np.inf,
                                                                             -b.dense[k]))[1])


def test_other_forms_of_the_operand(sh):
    """One torch.sparse_csr tensor in place of the triple, int32 crow, int64
    col_indices, and integer and 16-bit values (converted to float64)."""
    nr, nc = 100, 257
    b = S.batch("band_5pct", nr, nc)
    B = len(b.dense)
    crow, idx, val = device_csr(b)
    want = sh.solve_batched_sparse(crow, idx, val, shape=(B, nr, nc), duals=True)
    assert np.array_equal(want[0].cpu().numpy(), S.expected("band_5pct", nr, nc)[0])
    A = torch.sparse_csr_tensor(crow, idx.long(), val, size=(B * nr, nc))
    for got in (sh.solve_batched_sparse(A, shape=(B, nr, nc), duals=True),
                sh.solve_batched_sparse(crow.int(), idx.long(), val, shape=(B, nr, nc), duals=True),
                sh.solve_batched_sparse(crow, idx, val.long(), shape=(B, nr, nc), duals=True),
                sh.solve_batched_sparse(crow, idx, val.to(torch.int8), shape=(B, nr, nc), duals=True),
                sh.solve_batched_sparse(crow, idx, val.half(), shape=(B, nr, nc), duals=True),
                sh.solve_batched_sparse(crow, idx, val.bfloat16(), shape=(B, nr, nc), duals=True)):
        assert torch.equal(got[0], want[0]) and all(same_bits(g, w) for g, w in zip(got[1:], want[1:]))
    one = sh.solve_batched_sparse(torch.sparse_csr_tensor(crow[:nr + 1], idx[:int(crow[nr])].long(),
                                                          val[:int(crow[nr])], size=(nr, nc)))
    assert torch.equal(one[0], want[0][:1]) and same_bits(one[1], want[1][:1])


@pytest.mark.parametrize("family,nr,nc", [("band_5pct", 63, 65), ("explicit_zero", 64, 64), ("word_edges", 40, 2049),
                                          ("band_3", 3, 5)])
def test_linear_sum_assignment_sparse_is_scipys_dense_result(sh, family, nr, nc):
    sp = pytest.importorskip("scipy.sparse")
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    g = S.instance(family, nr, nc, 3)
    A = sp.csr_matrix((g.data, g.indices, g.indptr), shape=(nr, nc))
    assert A.nnz == g.data.size  # (stored zeros stay stored)
    for M, D in ((A, g.dense), (A.T, g.dense.T), (A.tocoo(), g.dense), (A.T.tocsr(), g.dense.T)):
        wr, wc = lsa(D)
        r, c = sh.linear_sum_assignment_sparse(M)
        assert r.dtype == np.int64 and c.dtype == np.int64
        assert np.array_equal(r, wr) and np.array_equal(c, wc), (family, M.shape)
        r2, c2, u, v = sh.linear_sum_assignment_sparse(M, duals=True)
        assert np.array_equal(r2, wr) and np.array_equal(c2, wc) and u.shape == (M.shape[0],) and v.shape == (M.shape[1],)
        slack = D - u[:, None] - v[None, :]  # (small integers: exact)
        assert (slack >= 0).all() and not slack[wr, wc].any()
        wr, wc = lsa(np.where(np.isinf(D), -np.inf, D), maximize=True)
        r, c = sh.linear_sum_assignment_sparse(M, maximize=True)
        assert np.array_equal(r, wr) and np.array_equal(c, wc), (family, M.shape, "maximize")
    r, c = sh.linear_sum_assignment_sparse((g.indptr, g.indices, g.data, (nr, nc)))
    assert np.array_equal(c, lsa(g.dense)[1])
    r, c = sh.linear_sum_assignment_sparse(torch.sparse_csr_tensor(torch.from_numpy(g.indptr),
                                                                   torch.from_numpy(g.indices).long(),
                                                                   torch.from_numpy(g.data), size=(nr, nc)))
    assert np.array_equal(c, lsa(g.dense)[1])


def test_linear_sum_assignment_sparse_raises_on_infeasible_input(sh):
    sp = pytest.importorskip("scipy.sparse")
    for family in ("hall", "empty_row"):
        g = S.instance(family, 63, 65, 0)
        A = sp.csr_matrix((g.data, g.indices, g.indptr), shape=(63, 65))
        for M in (A, A.T):
            with pytest.raises(ValueError, match="cost matrix is infeasible"):
                sh.linear_sum_assignment_sparse(M)
