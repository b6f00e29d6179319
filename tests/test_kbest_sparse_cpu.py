"""The k best assignments on sparse (CSR) costs, on the CPU (no GPU calls): the
family of tests/kbest_sparse_families.py against brute force through the
reference of tests/kbest_ref.py, a child's masked CSR written out by hand
against kbest_ref.masked, the lsap_murty_children_csr_ and lsap_kbest_csr_
entries' declarations and host checks, the Python front ends' argument errors
and empty-batch answers, and the new kernels in the built code object.
"""
import ctypes

import numpy as np
import pytest
import torch

import kbest_families as KF
import kbest_ref as KR
import kbest_sparse_families as KS
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions
from test_kernel_resources_cpu import _kernel_meta

SUFFIXES = ("f64", "f32")


# --------------------------------------------------------------------------- the family and the reference
def test_family_is_canonical_and_densifies_to_its_dense():
    for g in KS.family():
        nr, nc = g.shape
        assert g.indptr[0] == 0 and g.indptr[-1] == g.indices.size == g.data.size and g.indptr.size == nr + 1
        for i in range(nr):
            row = g.indices[g.indptr[i]:g.indptr[i + 1]]
            assert (np.diff(row) > 0).all() and ((row >= 0) & (row < nc)).all(), g.name
        D = lsap.densify(g.indptr, g.indices, g.data, g.shape)[:g.corner[0], :g.corner[1]]
        assert np.array_equal(D, g.dense), g.name
    names = [g.name for g in KS.family()]
    assert any(np.isinf(g.data).any() for g in KS.family()), "no stored +inf"
    assert any(g.corner != g.shape and g.indices.size and g.indices.max() >= g.corner[1] for g in KS.family())
    assert len(set(names)) == len(names)


def test_reference_on_the_densifications_against_brute_force():
    full = short = none = 0
    for g in KS.family():
        nr, nc = g.dense.shape
        if nr == 0:
            continue
        want = KF.brute_force(g.dense)
        cols, costs, count, _, _ = KR.kbest(g.dense, KS.K)
        assert count == min(KS.K, want.size), g.name
        assert np.array_equal(costs[:count], want[:count]), g.name
        KF.check_assignments(g.dense, cols, costs, count)  # (a finite chosen cost: a stored entry)
        for r in range(count):
            assert np.isfinite(g.dense[np.arange(nr), cols[r]]).all(), (g.name, r)
        full += count == KS.K
        short += 0 < count < KS.K
        none += count == 0
    assert full and short and none, (full, short, none)


def test_the_counts_that_are_known_in_closed_form():
    fib = {1: 1, 2: 2, 3: 3, 4: 5, 5: 8}
    by_name = {g.name: g for g in KS.family()}
    for n, f in fib.items():
        assert KF.brute_force(by_name[f"tridiagonal{n}"].dense).size == f
    assert KF.brute_force(by_name["bidiagonal4"].dense).size == 1
    assert KF.brute_force(by_name["empty_row"].dense).size == 0 and KF.brute_force(by_name["hall"].dense).size == 0


def test_masked_csr_written_out_by_hand_is_the_masked_densification():
    seen = 0
    for g in KS.family():
        nr, nc = g.shape
        if g.corner != g.shape or nr == 0:
            continue
        rng = np.random.default_rng([3, nr, nc])
        col = rng.permutation(nc)[:nr]
        for p in range(nr):
            F = rng.random(nc) < 0.3
            for t in range(p, nr):
                Ft = KR.forbidden_t(col, p, F, t)
                ip, ix, va = KS.masked_csr(g.indptr, g.indices, g.data, col, t, Ft)
                assert np.array_equal(lsap.densify(ip, ix, va, g.shape), KR.masked(g.dense, col, t, Ft)), (g.name, p, t)
                seen += 1
    assert seen > 100


# --------------------------------------------------------------------------- the C-ABI
def test_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    for suf in SUFFIXES:
        for name in (f"lsap_murty_children_csr_{suf}", f"lsap_kbest_csr_{suf}"):
            assert name in names and hasattr(L, name), name
        assert _lib.SIGNATURES[f"lsap_murty_children_csr_{suf}"] == \
            (I, [P, P, P, I, I, I, P, P, P, P, P, P, P, P, P, P, P, Z, U, P])
        assert _lib.SIGNATURES[f"lsap_kbest_csr_{suf}"] == (I, [P, P, P, I, I, I, P, I, P, P, P, P, Z, U, P])
    assert "lsap_kbest_csr_work_bytes" in names
    assert _lib.SIGNATURES["lsap_kbest_csr_work_bytes"] == (Z, [I, I, I, I])
    import santa_hip
    for name in ("kbest_batched_sparse", "kbest_assignments_sparse", "murty_children_batched_sparse"):
        assert hasattr(santa_hip, name) and name in santa_hip.__all__, name


def _p(x):
    return ctypes.c_void_p(x) if x else None  # (never dereferenced)


def _children(suf, nr, nc, B, work=0x1000, work_bytes=1 << 40, indices=0x1000, data=0x1000, **null):
    a = {k: 0x1000 for k in ("indptr", "pcol", "pv", "p", "forb", "col", "cost", "u", "v")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_murty_children_csr_" + suf)(
        _p(a["indptr"]), _p(indices), _p(data), nr, nc, B, None, _p(a["pcol"]), _p(a["pv"]), _p(a["p"]),
        _p(a["forb"]), _p(a["col"]), _p(a["cost"]), _p(a["u"]), _p(a["v"]), None, _p(work), work_bytes, 0, None)


def _kbest(suf, nr, nc, B, k, work=0x1000, work_bytes=1 << 40, flags=0, indices=0x1000, data=0x1000, **null):
    a = {k_: 0x1000 for k_ in ("indptr", "cols", "costs", "count")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_kbest_csr_" + suf)(
        _p(a["indptr"]), _p(indices), _p(data), nr, nc, B, None, k, _p(a["cols"]), _p(a["costs"]), _p(a["count"]),
        _p(work), work_bytes, flags, None)


@pytest.mark.parametrize("suf", SUFFIXES)
def test_children_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    assert _children(suf, 0, 5, 1) == E
    assert _children(suf, 6, 5, 1) == E
    assert "transpose" in _lib.last_error()
    assert _children(suf, 5, _lib.SH_MAX_N + 1, 1) == E
    assert "1024" in _lib.last_error()
    assert _children(suf, 3, 5, -1) == E
    assert _children(suf, 1024, 1024, (1 << 21) + 1) == E
    assert "2^31" in _lib.last_error()
    for null in ("indptr", "pcol", "pv", "p", "forb", "col", "cost", "u", "v"):
        assert _children(suf, 3, 5, 1, **{null: 0}) == E, null
    need = _lib.lib().lsap_csr_work_bytes(3, 5, 2)
    assert _children(suf, 3, 5, 2, work_bytes=need - 1) == E
    assert "lsap_csr_work_bytes" in _lib.last_error()
    assert _children(suf, 3, 5, 2, work=0) == E
    assert _children(suf, 3, 5, 2, work=0x1004) == E
    assert "aligned" in _lib.last_error()
    assert _children(suf, 3, 5, 0) == _lib.SH_OK
    assert _children(suf, 1024, 1024, 0, work=0, work_bytes=0, indices=0, data=0, indptr=0, pcol=0, pv=0, p=0, forb=0,
                     col=0, cost=0, u=0, v=0) == _lib.SH_OK
    assert _children(suf, 6, 5, 0) == E


@pytest.mark.parametrize("suf", SUFFIXES)
def test_kbest_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    need = _lib.lib().lsap_kbest_csr_work_bytes(3, 5, 2, 4)
    assert need > 0 and need % 8 == 0
    assert _kbest(suf, 0, 5, 1, 4) == E
    assert _kbest(suf, 6, 5, 1, 4) == E
    assert "transpose" in _lib.last_error()
    assert _kbest(suf, 5, _lib.SH_MAX_N + 1, 1, 4) == E
    assert "1024" in _lib.last_error()
    assert _kbest(suf, 3, 5, -1, 4) == E
    assert _kbest(suf, 3, 5, 2, 0) == E
    assert "k < 1" in _lib.last_error()
    assert _kbest(suf, 1024, 1024, (1 << 21) + 1, 4) == E  # B * nr
    assert "2^31" in _lib.last_error()
    assert _kbest(suf, 1024, 1024, 1, (1 << 21) + 1) == E  # k * nr
    assert "k * nr" in _lib.last_error()
    for null in ("indptr", "cols", "costs", "count"):
        assert _kbest(suf, 3, 5, 2, 4, **{null: 0}) == E, null
    assert _kbest(suf, 3, 5, 2, 4, work=0) == E
    assert _kbest(suf, 3, 5, 2, 4, work_bytes=need - 1) == E
    assert "work_bytes" in _lib.last_error()
    assert _kbest(suf, 3, 5, 2, 4, work_bytes=_lib.lib().lsap_kbest_work_bytes(3, 5, 2, 4)) == E  # the dense pool alone
    assert _kbest(suf, 3, 5, 2, 4, work=0x1004, work_bytes=need) == E
    assert "aligned" in _lib.last_error()
    assert _kbest(suf, 3, 5, 2, 4, flags=_lib.SH_FLAG_F64_MW | _lib.SH_FLAG_F64_SW) == E
    assert "exclude" in _lib.last_error()
    assert _kbest(suf, 3, 5, 0, 4, work=0x1004, work_bytes=0) == E  # (the alignment is checked for B == 0 too)
    assert _kbest(suf, 3, 5, 0, 4) == _lib.SH_OK
    assert _kbest(suf, 3, 5, 0, 4, work=0, work_bytes=0, indices=0, data=0, indptr=0, cols=0, costs=0,
                  count=0) == _lib.SH_OK
    assert _kbest(suf, 6, 5, 0, 4) == E


def test_work_bytes_is_the_dense_pool_plus_the_csr_words():
    L = _lib.lib()
    f = L.lsap_kbest_csr_work_bytes
    for nr, nc, B in ((1, 1, 1), (3, 5, 2), (64, 64, 7), (250, 257, 3), (1024, 1024, 1)):
        sizes = [f(nr, nc, B, k) for k in (1, 2, 3, 10, 100)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (nr, nc, B, sizes)
        for k, s in zip((1, 2, 3, 10, 100), sizes):
            want = L.lsap_kbest_work_bytes(nr, nc, B, k) + L.lsap_csr_work_bytes(nr, nc, B)
            assert s == (want + 7) // 8 * 8, (nr, nc, B, k)
    for bad in ((0, 5, 1, 3), (6, 5, 1, 3), (5, 1025, 1, 3), (3, 5, -1, 3), (3, 5, 1, 0), (3, 5, 1, -2),
                (1024, 1024, (1 << 21) + 1, 1)):
        assert f(*bad) == 0, bad
    assert f(3, 5, 0, 3) == 0  # (no instance: nothing to hold)
    assert f(1024, 1024, 1 << 20, 1 << 30) == 0  # (does not fit a size_t: rejected, not wrapped)


# --------------------------------------------------------------------------- the code object
FORBIDDEN = ("lsap_", "murty_", "kbest_", "warm_csr_", "csr_cert_kernel", "csr_slack_kernel", "csr_edges_kernel",
             "csr_match_kernel", "csr_hall_check_kernel")


def test_new_kernels_exist_use_no_scratch_and_are_the_launch_table(tmp_path):
    meta = _kernel_meta(tmp_path)
    new = {k: v for k, v in meta.items() if "mcsr_" in k}
    assert not [(k, s) for k in new for s in FORBIDDEN if s in k], "a new kernel's name moves an existing count"
    assert not {k: v for k, v in new.items() if v}, "kernels with private (scratch) memory"
    assert sum("mcsr_prep_kernelId" in k for k in new) == 1 and sum("mcsr_prep_kernelIf" in k for k in new) == 1
    # one wave (one column a thread) up to 64 columns; four waves, 10-bit keys, 1 / 2 / 4 columns a thread beyond
    want = {f"mcsr_f64_kernelILi1E{s}E" for s in "df"}
    want |= {f"mcsr_f64_mw_kernelILi4ELi{k}E{s}Li10EE" for k in (1, 2, 4) for s in "df"}
    cont = [k for k in new if "mcsr_f64_" in k]
    assert len(cont) == 8 and len(want) == 8
    for w in want:
        assert sum(w in k for k in cont) == 1, w
    assert len(new) == 10


# --------------------------------------------------------------------------- the front ends
@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise AssertionError("a host check should have answered first")
    monkeypatch.setattr(lsap, "require_gpu", refuse)


def _triple(B=2, NR=3, NC=4):
    crow = torch.arange(0, B * NR + 1, dtype=torch.int64)  # one entry a row, on column r % NC
    idx = (torch.arange(B * NR) % NC).to(torch.int32)
    return crow, idx, torch.ones(B * NR, dtype=torch.float64)


def test_kbest_batched_sparse_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.kbest_batched_sparse
    crow, idx, val = _triple()
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            f(crow, idx, val, (2, 3, 4), k=k)
    with pytest.raises(ValueError, match=r"\(B, NR, NC\)"):
        f(crow, idx, val, (6, 4), k=2)
    with pytest.raises(ValueError, match="must be wide"):
        f(crow, idx, val, (2, 3, 2), k=2)
    with pytest.raises(ValueError, match="crow"):
        f(crow[:-1], idx, val, (2, 3, 4), k=2)
    with pytest.raises(ValueError, match="strictly increasing"):
        f(torch.tensor([0, 2, 2, 2, 2, 2, 2]), torch.tensor([1, 1], dtype=torch.int32), val[:2], (2, 3, 4), k=2)
    with pytest.raises(TypeError, match="unsupported"):
        f(crow, idx, val.to(torch.complex64), (2, 3, 4), k=2)
    with pytest.raises(ValueError, match="1024"):
        f(torch.zeros(3, dtype=torch.int64), idx[:0], val[:0], (1, 2, 1025), k=2)
    with pytest.raises(ValueError, match="transpose"):
        f(crow, idx, val, (2, 3, 4), k=2, shapes=[[3, 4], [3, 2]])
    A = torch.sparse_csr_tensor(crow, idx, val, size=(6, 4))
    with pytest.raises(ValueError, match="no batch of shape"):
        f(A, shape=(2, 3, 5), k=2)
    with pytest.raises(ValueError, match="k must be"):  # the sparse tensor in place of the triple reaches the k check
        f(A, shape=(2, 3, 4), k=0)


def test_a_pool_that_does_not_fit_raises(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    B, NR, NC = 1, 1024, 1024
    crow = torch.zeros(B * NR + 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="too large"):
        lsap.kbest_batched_sparse(crow, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64),
                                  (B, NR, NC), k=(1 << 21) + 1, validate=False)


def test_murty_children_batched_sparse_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.murty_children_batched_sparse
    crow, idx, val = _triple()
    val = val.float()
    col, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.float64)
    p, forb = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ValueError, match="expected col"):
        f(crow, idx, val, (2, 3, 4), col[:, :2], v, p, forb)
    with pytest.raises(ValueError, match="expected col"):
        f(crow, idx, val, (2, 3, 4), col, v, p, torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(TypeError, match="float64"):
        f(crow, idx, val, (2, 3, 4), col, v.float(), p, forb)
    with pytest.raises(TypeError, match="int64"):
        f(crow, idx, val, (2, 3, 4), col, v, p, forb.to(torch.int32))
    with pytest.raises(TypeError, match="integer"):
        f(crow, idx, val, (2, 3, 4), col.double(), v, p, forb)
    with pytest.raises(ValueError, match="must be wide"):
        f(crow, idx, val, (2, 3, 2), col, v, p, forb)
    with pytest.raises(ValueError, match="1024"):
        f(torch.zeros(3, dtype=torch.int64), idx[:0], val[:0], (1, 2, 1025), col[:1, :2],
          torch.zeros((1, 1025), dtype=torch.float64), p[:1], torch.zeros((1, 17), dtype=torch.int64))
    with pytest.raises(ValueError, match="strictly increasing"):
        f(torch.tensor([0, 2, 2, 2, 2, 2, 2]), torch.tensor([1, 1], dtype=torch.int32), val[:2], (2, 3, 4), col, v, p,
          forb)


def test_empty_batches(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    inf = float("inf")
    for shape in ((0, 3, 4), (2, 0, 4), (0, 0, 0)):
        B, NR, NC = shape
        crow, idx = torch.zeros(B * NR + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
        for dt in (torch.float64, torch.float32):
            val = torch.zeros(0, dtype=dt)
            for maximize in (False, True):
                cols, costs, count = lsap.kbest_batched_sparse(crow, idx, val, shape, k=5, maximize=maximize)
                assert tuple(cols.shape) == (B, 5, NR) and cols.dtype == torch.int32 and bool((cols == -1).all())
                assert tuple(costs.shape) == (B, 5) and costs.dtype == torch.float64
                assert bool((costs == (-inf if maximize else inf)).all())
                assert tuple(count.shape) == (B,) and count.dtype == torch.int32 and not count.any()
            col, cost, u, v, kept = lsap.murty_children_batched_sparse(
                crow, idx, val, shape, torch.zeros((B, NR), dtype=torch.int32), torch.zeros((B, NC), dtype=torch.float64),
                torch.zeros(B, dtype=torch.int32), torch.zeros((B, (NC + 63) // 64), dtype=torch.int64))
            assert tuple(col.shape) == (B, NR, NR) and bool((col == -1).all())
            assert tuple(cost.shape) == (B, NR) and bool((cost == inf).all())
            assert tuple(u.shape) == (B, NR, NR) and tuple(v.shape) == (B, NR, NC) and tuple(kept.shape) == (B, NR)
            assert not u.any() and not v.any() and not kept.any()


def test_single_matrix_front_end_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.kbest_assignments_sparse
    A = (np.array([0, 1, 2, 3]), np.array([0, 1, 2], dtype=np.int32), np.ones(3), (3, 4))
    for k in (0, -3, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            f(A, k)
    with pytest.raises(ValueError, match="1024"):
        f((np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (2, 1025)), 2)
    with pytest.raises(ValueError, match="1024"):
        f((np.zeros(1026, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (1025, 2)), 2)
    with pytest.raises(ValueError, match="sparse_csr"):
        f(torch.zeros((3, 4)), 2)
    with pytest.raises(ValueError, match="invalid numeric"):
        f((A[0], A[1], np.array([1.0, np.nan, 2.0]), A[3]), 2)
    with pytest.raises(ValueError, match="invalid numeric"):
        f((A[0], A[1], np.array([1.0, -np.inf, 2.0]), A[3]), 2)
    with pytest.raises(ValueError, match="invalid numeric"):
        f((A[0], A[1], np.array([1.0, np.inf, 2.0]), A[3]), 2, maximize=True)
    cols, costs = f((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (0, 4)), 3)
    assert cols.shape == (0, 0) and cols.dtype == np.int64 and costs.shape == (0,) and costs.dtype == np.float64
    cols, costs = f((np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (3, 0)), 3)
    assert cols.shape == (0, 3) and costs.shape == (0,)
