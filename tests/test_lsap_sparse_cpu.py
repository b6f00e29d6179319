"""CPU tests of the sparse (CSR) batched LSAP surface: the library's exports
and host checks (no GPU is touched: every call is turned down on the host or
has B == 0), the pure helpers of santa_hip.lsap (validate_csr, csr_transpose,
densify) against scipy.sparse, and the expectations of the GPU tests -- for
every family and shape of lsap_sparse_families the oracle is feasible or not as
the family says, and the replay of scipy's loop agrees with it."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_duals_ref as R  # noqa: E402
import lsap_sparse_families as S  # noqa: E402
import oracle  # noqa: E402
from santa_hip import _lib, lsap  # noqa: E402

ENTRIES = ("lsap_solve_csr_f64", "lsap_solve_csr_f32")


def _ptr(x=4096):
    """A non-null pointer the entry never dereferences."""
    return ctypes.c_void_p(x)


def _solve(name, nr, nc, B, indptr=True, col=True, cost=True, u=True, v=True, work=True, work_bytes=None, flags=0):
    p = lambda on: _ptr() if on else None  # noqa: E731
    if work_bytes is None:
        work_bytes = _lib.lib().lsap_csr_work_bytes(nr, nc, B)
    return getattr(_lib.lib(), name)(p(indptr), _ptr(), _ptr(), nr, nc, B, None, p(col), p(cost), p(u), p(v),
                                     p(work), work_bytes, flags, None)


def test_library_exports_the_three_symbols():
    L = _lib.lib()
    for name in ENTRIES + ("lsap_csr_work_bytes",):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["lsap_csr_work_bytes"][0] is ctypes.c_size_t
    import santa_hip
    for name in ("solve_batched_sparse", "linear_sum_assignment_sparse", "densify", "csr_transpose", "validate_csr"):
        assert getattr(santa_hip, name) is getattr(lsap, name) and name in santa_hip.__all__


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_check_their_arguments_on_the_host(name):
    E, OK = _lib.SH_ERR_ARGS, _lib.SH_OK
    MW, SW = _lib.SH_FLAG_F64_MW, _lib.SH_FLAG_F64_SW
    assert _solve(name, 0, 10, 1) == E
    assert _solve(name, -1, 10, 1) == E
    assert _solve(name, 11, 10, 1) == E and "nr > nc" in _lib.last_error()
    assert _solve(name, 10, 4097, 1) == E and "4096" in _lib.last_error()
    assert _solve(name, 10, 2000, -1) == E and "B < 0" in _lib.last_error()
    assert _solve(name, 10, 2000, 1, indptr=False) == E and "indptr" in _lib.last_error()
    assert _solve(name, 10, 2000, 1, col=False) == E
    assert _solve(name, 10, 2000, 1, u=False) == E and "both or neither" in _lib.last_error()
    assert _solve(name, 10, 100, 1, v=False) == E
    need = _lib.lib().lsap_csr_work_bytes(10, 2000, 3)
    assert need > 0
    assert _solve(name, 10, 2000, 3, work_bytes=need - 1) == E and "work" in _lib.last_error()
    assert _solve(name, 10, 2000, 3, work_bytes=0) == E
    assert _solve(name, 10, 2000, 3, work=False) == E
    for nc in (100, 1024, 1025, 4096):
        assert _solve(name, 10, nc, 1, flags=MW | SW) == E and "exclude" in _lib.last_error()
        assert _solve(name, 10, nc, 0, flags=MW | SW) == E
    assert _solve(name, 10, 1025, 1, flags=SW) == E and "one-wave" in _lib.last_error()
    # the checks come first for B == 0 too; then nothing is needed
    assert _solve(name, 10, 4097, 0) == E and _solve(name, 11, 10, 0) == E
    assert _solve(name, 10, 4096, 0, flags=SW) == E
    assert _solve(name, 10, 1024, 0, flags=SW) == OK and _solve(name, 10, 4096, 0, flags=MW) == OK
    assert _solve(name, 4096, 4096, 0) == OK
    assert _solve(name, 1, 1, 0, indptr=False, col=False, cost=False, u=False, v=False, work=False) == OK


def test_work_bytes_is_monotone_in_each_argument():
    wb = _lib.lib().lsap_csr_work_bytes
    assert wb(0, 10, 1) == 0 and wb(10, 10, 0) == 0 and wb(10, 0, 1) == 0
    sizes = (1, 2, 63, 64, 65, 128, 129, 1000, 1024, 1025, 4095, 4096)
    for a in sizes:
        for lo, hi in zip(sizes, sizes[1:]):
            assert 0 < wb(lo, 4096, a) <= wb(hi, 4096, a)
            assert 0 < wb(a, max(a, lo), 7) <= wb(a, max(a, hi), 7)
            assert 0 < wb(a, 4096, lo) <= wb(a, 4096, hi)
    # ten bytes per row and 64-column word, and room for the largest batch of the measurements
    assert wb(4096, 4096, 256) == 256 * 4096 * 64 * 10
    assert wb(1, 1, 1) >= 10 and wb(1, 64, 1) == wb(1, 1, 1) and wb(1, 65, 1) > wb(1, 64, 1)


# --------------------------------------------------------------------------- validate
def _good():
    # 2 instances of 2 x 4: rows {0, 2}, {1}, {}, {0, 1, 3}
    return (torch.tensor([0, 2, 3, 3, 6]), torch.tensor([0, 2, 1, 0, 1, 3], dtype=torch.int32),
            torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=torch.float64))


def test_validate_accepts_canonical_input_and_rejects_each_malformation():
    shape = (2, 2, 4)
    crow, idx, val = _good()
    lsap.validate_csr(crow, idx, val, shape)
    lsap.validate_csr(crow.int(), idx.long(), val.float(), shape)
    lsap.validate_csr(torch.zeros(5, dtype=torch.int64), idx[:0], val[:0], shape)  # no entry at all
    inf = val.clone()
    inf[2] = float("inf")  # (a stored +inf is a missing entry, not an error)
    lsap.validate_csr(crow, idx, inf, shape)

    def bad(match, crow=crow, idx=idx, val=val, **kw):
        with pytest.raises(ValueError, match=match):
            lsap.validate_csr(crow, idx, val, shape, **kw)

    bad(r"crow\[0\]", crow=torch.tensor([1, 2, 3, 3, 6]))
    bad("decreasing", crow=torch.tensor([0, 3, 2, 3, 6]))
    bad(r"crow\[-1\]", crow=torch.tensor([0, 2, 3, 3, 5]))
    bad(r"crow\[-1\]", crow=torch.tensor([0, 2, 3, 3, 7]))
    bad("entries", crow=torch.tensor([0, 2, 3, 6]))
    bad("equal length", val=val[:5])
    bad("outside", idx=torch.tensor([0, 4, 1, 0, 1, 3], dtype=torch.int32))
    bad("outside", idx=torch.tensor([-1, 2, 1, 0, 1, 3], dtype=torch.int32))
    bad("strictly increasing", idx=torch.tensor([2, 0, 1, 0, 1, 3], dtype=torch.int32))
    bad("strictly increasing", idx=torch.tensor([0, 2, 1, 0, 1, 1], dtype=torch.int32))  # a duplicate
    nan, ninf = val.clone(), val.clone()
    nan[4] = float("nan")
    ninf[0] = float("-inf")
    bad("invalid numeric", val=nan)
    bad("invalid numeric", val=ninf)
    # entry 4 is (instance 1, row 1, column 1): outside a (1, 4) or a (2, 1) corner it is never used
    lsap.validate_csr(crow, idx, nan, shape, shapes=np.array([[2, 4], [1, 4]]))
    lsap.validate_csr(crow, idx, nan, shape, shapes=np.array([[2, 4], [1, 1]]))
    bad("invalid numeric", val=nan, shapes=np.array([[1, 1], [2, 4]]))
    # a decrease across a row boundary is no error: rows {0, 2}, {1}
    lsap.validate_csr(torch.tensor([0, 2, 3]), torch.tensor([0, 2, 1]), val[:3], (1, 2, 4))


def test_front_end_checks_before_the_device(monkeypatch):
    crow, idx, val = _good()
    with pytest.raises(ValueError, match="wide"):
        lsap.solve_batched_sparse(crow, idx, val, shape=(1, 4, 3))
    with pytest.raises(ValueError, match="4096"):
        lsap.solve_batched_sparse(crow, idx, val, shape=(2, 2, 4097))
    with pytest.raises(ValueError, match="shape"):
        lsap.solve_batched_sparse(crow, idx, val)
    with pytest.raises(ValueError, match="strictly increasing"):
        lsap.solve_batched_sparse(crow, torch.tensor([2, 0, 1, 0, 1, 3]), val, shape=(2, 2, 4))
    with pytest.raises(ValueError, match="outside the padded"):
        lsap.solve_batched_sparse(crow, idx, val, shape=(2, 2, 4), shapes=[(1, 5), (1, 1)])
    with pytest.raises(TypeError):
        lsap.solve_batched_sparse(crow, idx, val.to(torch.complex64), shape=(2, 2, 4))
    A = torch.sparse_csr_tensor(crow, idx.long(), val, size=(4, 4))
    with pytest.raises(ValueError, match="no batch of shape"):
        lsap.solve_batched_sparse(A, shape=(2, 3, 4))
    # empty batches need no device
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    col, cost, u, v = lsap.solve_batched_sparse(torch.zeros(1, dtype=torch.int64), idx[:0], val[:0],
                                                shape=(0, 5, 7), duals=True)
    assert tuple(col.shape) == (0, 5) and tuple(cost.shape) == (0,) and tuple(v.shape) == (0, 7)
    # the single-matrix front end: empty input, size limit, and the route to the batched solve
    for shape in ((0, 0), (0, 5), (5, 0)):
        z = lsap.linear_sum_assignment_sparse((np.zeros(shape[0] + 1, dtype=np.int64), [], [], shape), device="cpu",
                                              duals=True)
        assert [a.size for a in z] == [0, 0, shape[0], shape[1]]
    with pytest.raises(ValueError, match="4096"):
        lsap.linear_sum_assignment_sparse((np.zeros(3, dtype=np.int64), [], [], (2, 4097)), device="cpu")
    seen = []

    def fake(crow, col_indices, values, shape, with_cost, maximize, duals):
        seen.append((shape, values.dtype, maximize))
        D = lsap.densify(crow, col_indices, -values if maximize else values, shape)[0]
        colr, u, v = R.replay(D)
        out = (torch.from_numpy(colr.astype(np.int32))[None], None)
        return out + ((torch.from_numpy(-u if maximize else u)[None], torch.from_numpy(-v if maximize else v)[None])
                      if duals else ())

    monkeypatch.setattr(lsap, "solve_batched_sparse", fake)
    sp = pytest.importorskip("scipy.sparse")
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(5)
    for shape in ((6, 9), (9, 6), (5, 5)):
        M = rng.integers(1, 50, size=shape) * (rng.random(shape) < 0.6)
        M[np.arange(min(shape)), np.arange(min(shape))] = 7
        D = np.where(M != 0, M.astype(np.float64), np.inf)
        for A in (sp.csr_matrix(M), sp.coo_matrix(M), sp.csc_matrix(M.astype(np.float32)),
                  torch.from_numpy(M.astype(np.float64)).to_sparse_csr()):
            r, c, u, v = lsap.linear_sum_assignment_sparse(A, device="cpu", duals=True)
            wr, wc = lsa(D)
            assert np.array_equal(r, wr) and np.array_equal(c, wc), shape
            assert seen[-1][0] == (1, min(shape), max(shape))
            assert u.shape == (shape[0],) and v.shape == (shape[1],)
            assert np.all(D - u[:, None] - v[None, :] >= 0) and not (D - u[:, None] - v[None, :])[r, c].any()
        r, c = lsap.linear_sum_assignment_sparse(sp.csr_matrix(M), maximize=True, device="cpu")
        wr, wc = lsa(np.where(M != 0, M.astype(np.float64), -np.inf), maximize=True)
        assert np.array_equal(r, wr) and np.array_equal(c, wc) and seen[-1][2] is True


# --------------------------------------------------------------------------- helpers against scipy.sparse
def test_csr_transpose_and_densify_agree_with_scipy_sparse():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(11)
    for nr, nc, p in ((1, 1, 1.0), (7, 3, 0.5), (3, 7, 0.5), (40, 130, 0.1), (130, 40, 0.02), (5, 5, 0.0)):
        M = sp.random(nr, nc, density=p, format="csr", random_state=rng, dtype=np.float64)
        M.sort_indices()
        D = lsap.densify(M.indptr, M.indices, M.data, (nr, nc))
        W = np.full((nr, nc), np.inf)
        W[M.nonzero()] = M.data  # (sp.random stores no zero)
        assert np.array_equal(D, W)
        ip, ix, dt, shape = lsap.csr_transpose(M.indptr, M.indices, M.data, (nr, nc))
        T = M.T.tocsr()
        T.sort_indices()
        assert shape == (nc, nr) and ip.dtype == np.int64
        assert np.array_equal(ip, T.indptr) and np.array_equal(ix, T.indices) and np.array_equal(dt, T.data)
        assert np.array_equal(lsap.densify(ip, ix, dt, shape), D.T)
    # a batch: B * NR rows reshaped, torch input, narrow values widened
    g = S.batch("band_5pct", 3, 5)
    D = lsap.densify(torch.from_numpy(g.indptr), torch.from_numpy(g.indices),
                     torch.from_numpy(g.data).to(torch.bfloat16), (8, 3, 5))
    assert D.dtype == np.float64 and np.array_equal(D, np.stack(g.dense))


# --------------------------------------------------------------------------- the families pin the GPU tests' expectations
def test_families_are_canonical_and_hold_what_they_name():
    for family, nr, nc in S.cases():
        b = S.batch(family, nr, nc)
        B = S.batch_size(nc)
        lsap.validate_csr(torch.from_numpy(b.indptr), torch.from_numpy(b.indices), torch.from_numpy(b.data),
                          (B, nr, nc), shapes=np.array(b.corners) if b.corners else None)
        fin = b.data[np.isfinite(b.data)]
        assert ((fin >= 0) & (fin <= 63) & (fin == np.round(fin))).all(), (family, nr, nc)
        if not b.corners:
            assert np.array_equal(lsap.densify(b.indptr, b.indices, b.data, (B, nr, nc)), np.stack(b.dense))
    assert np.isnan(S.batch("ragged", 40, 129).data).any()
    assert np.isinf(S.batch("full", 64, 64).data).any()
    nnz = np.diff(S.batch("uneven", 100, 257).indptr[::100])
    assert nnz.min() == 0 and nnz.max() > 50 * max(1, np.sort(nnz)[1])
    # word_edges: rows confined to the last word, rows with an empty word between two populated ones
    for nr, nc in ((100, 257), (300, 300), (40, 4096)):
        P = np.isfinite(S.instance("word_edges", nr, nc, 0).dense)
        words = np.add.reduceat(P, np.arange(0, nc, 64), axis=1) > 0
        assert (words[:, -1] & ~words[:, :-1].any(axis=1)).any(), (nr, nc)
        gap = [(w[:-2] & ~w[1:-1] & w[2:]).any() for w in words]
        assert any(gap), (nr, nc)
    # explicit_zero: a stored zero read as missing, or a missing entry read as zero, changes col
    for nr, nc in ((3, 5), (64, 64), (100, 257)):
        D = S.instance("explicit_zero", nr, nc, 0).dense
        col = oracle.lsap(D)[1]
        assert (D == 0).any() and (D[np.arange(nr), col] == 0).any()
        assert not np.array_equal(oracle.lsap(np.where(D == 0, np.inf, D))[1], col)
        assert not np.array_equal(oracle.lsap(np.where(np.isinf(D), 0.0, D))[1], col)
    # bidiagonal: a dear row's Dijkstra walks back its whole run of 24 rows
    D = S.instance("bidiagonal", 64, 64, 0).dense
    col = oracle.lsap(D)[1]
    assert np.array_equal(col, np.arange(64))  # (square: the last row has one column, so the identity)
    assert np.array_equal(oracle.lsap(S.instance("bidiagonal", 63, 65, 0).dense)[1][:23], np.arange(23))


@pytest.mark.parametrize("family,nr,nc", S.cases())
def test_oracle_and_replay_agree_on_every_family(family, nr, nc):
    b = S.batch(family, nr, nc)
    for k, D in enumerate(b.dense):
        if D.shape[0] == 0:
            assert not b.feasible[k]
            continue
        if b.feasible[k]:
            col = oracle.lsap(D)[1]
            rcol, u, v = R.replay(D)
            assert np.array_equal(rcol, col), k
            assert np.isfinite(D[np.arange(D.shape[0]), col]).all()
            # (small integer costs: the float duals are integers, so the invariants hold exactly)
            slack = D - u[:, None] - v[None, :]
            assert (slack >= 0).all() and not slack[np.arange(D.shape[0]), col].any() and (v <= 0).all()
        else:
            with pytest.raises(ValueError, match="infeasible"):
                oracle.lsap(D)
            with pytest.raises(ValueError, match="infeasible"):
                R.replay(D)
    col, u, v = S.expected(family, nr, nc)
    for k in range(len(b.dense)):
        assert (col[k] >= 0).any() == (b.feasible[k] and b.dense[k].shape[0] > 0)
