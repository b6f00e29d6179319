"""The warm start of the sparse (CSR) batched LSAP solver on the CPU (no GPU
calls): the lsap_warm_csr_ entries' declarations and host checks, the
warm_csr_ kernels of the gfx950 code object, the Python front ends' argument
errors, and a proof that what tests/test_lsap_warm_sparse_gpu.py expects is not
vacuous.

The last part runs tests/lsap_warm_ref.py on the densifications of
tests/lsap_warm_sparse_families.py's cases, without the feature:

* every feasible unperturbed instance is a fixed point of the warm start from
  its own cold solution: kept == nr, no search, the same col;
* every perturbed instance that stays feasible ends with the cold replay's cost;
* over the case list there is at least one instance that is feasible with
  0 < kept < nr, one wide instance with kept < nr - 4 (the raise cascade), one
  made infeasible by the removed entry while every row keeps an edge (so the
  continuation, not the prologue, finds it) and one infeasible in the prologue.
"""
import ctypes

import numpy as np
import pytest
import torch

import lsap_sparse_families as S
import lsap_warm_ref as W
import lsap_warm_sparse_families as WS
import oracle
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions
from test_kernel_resources_cpu import _kernel_meta

ENTRIES = ("lsap_warm_csr_f64", "lsap_warm_csr_f32")


# --------------------------------------------------------------------------- the C-ABI
def test_warm_csr_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    header = open(__import__("test_cabi_cpu").HEADER).read()
    for name, data in zip(ENTRIES, ("const double *d_data", "const float *d_data")):
        assert name in names and hasattr(L, name), name
        # indptr, indices, data, nr, nc, B, shape, col, cost, u, v, kept, work, work_bytes, flags, stream
        assert _lib.SIGNATURES[name] == (I, [P, P, P, I, I, I, P, P, P, P, P, P, P, Z, U, P]), name
        decl = header[header.index(f"int {name}("):]
        decl = " ".join(decl[:decl.index(";")].split())
        assert decl.count(",") == 15 and data in decl, name
        assert "int32_t *d_kept, void *d_work, size_t work_bytes, unsigned flags, void *stream" in decl, name
    import santa_hip
    for name in ("resolve_batched_sparse", "linear_sum_assignment_sparse_resolve"):
        assert hasattr(santa_hip, name) and name in santa_hip.__all__, name


def _call(name, nr, nc, B, indptr=1, col=1, u=1, v=1, work=0x1000, work_bytes=None, indices=1, data=1):
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731  (never dereferenced)
    if work_bytes is None:
        work_bytes = _lib.lib().lsap_csr_work_bytes(nr, nc, B)
    return getattr(_lib.lib(), name)(p(indptr), p(indices), p(data), nr, nc, B, None, p(col), None, p(u), p(v), None,
                                     ctypes.c_void_p(work) if work else None, work_bytes, 0, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_warm_csr_host_checks_without_gpu(name):
    E = _lib.SH_ERR_ARGS
    assert _call(name, 0, 5, 1) == E
    assert _call(name, 6, 5, 1) == E
    assert "transpose" in _lib.last_error()
    assert _call(name, 5, _lib.SH_MAX_N_LARGE + 1, 1) == E
    assert "4096" in _lib.last_error()
    assert _call(name, 3, 5, -1) == E
    for null in ("indptr", "col", "u", "v"):
        assert _call(name, 3, 5, 1, **{null: 0}) == E, null
    need = _lib.lib().lsap_csr_work_bytes(3, 5, 2)
    assert need > 0
    assert _call(name, 3, 5, 2, work_bytes=need - 1) == E
    assert "lsap_csr_work_bytes" in _lib.last_error()
    assert _call(name, 3, 5, 2, work=0) == E
    assert _call(name, 3, 5, 2, work=0x1004) == E
    assert "aligned" in _lib.last_error()
    # B * nr too large for the grid of the pass over the CSR (four rows a workgroup)
    B = (1 << 31) // 1024 * 4 + 8
    assert B * 1024 // 4 > (1 << 31) - 1
    assert _call(name, 1024, 1024, B, work_bytes=1 << 62) == E
    assert "too large" in _lib.last_error()
    # B == 0 is a no-op after the checks; so are the size errors before it
    assert _call(name, 3, 5, 0) == _lib.SH_OK
    assert _call(name, 3, 5, 0, indptr=0, col=0, u=0, v=0, work=0, indices=0, data=0) == _lib.SH_OK
    assert _call(name, 4096, 4096, 0) == _lib.SH_OK
    assert _call(name, 6, 5, 0) == E


# --------------------------------------------------------------------------- the code object
def test_warm_csr_kernels_exist_and_use_no_scratch(tmp_path):
    meta = _kernel_meta(tmp_path)
    mine = {k: v for k, v in meta.items() if "warm_csr_" in k}
    assert not any("lsap_" in k for k in mine), "a warm_csr_ kernel's name would move the pinned lsap_ kernel set"
    prologues = [k for k in mine if "warm_csr_prep_kernel" in k]
    continuations = [k for k in mine if "warm_csr_kernel" in k or "warm_csr_mw_kernel" in k]
    assert len(prologues) == 2, prologues
    assert len(continuations) == 14, continuations  # 7 configurations x 2 storage types
    assert len(mine) == 16
    assert not {k: v for k, v in mine.items() if v}, "kernels with private (scratch) memory"


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


def test_resolve_batched_sparse_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.resolve_batched_sparse
    crow, idx, val = _triple()
    col = torch.zeros((2, 3), dtype=torch.int32)
    u, v = torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\(B, NR, NC\)"):
        f(crow, idx, val, (6, 4), col, u, v)
    with pytest.raises(ValueError, match="must be wide"):
        f(crow, idx, val, (2, 3, 2), col, u, v)
    with pytest.raises(ValueError, match="crow"):
        f(crow[:-1], idx, val, (2, 3, 4), col, u, v)
    with pytest.raises(ValueError, match="strictly increasing"):
        f(torch.tensor([0, 2, 2, 2, 2, 2, 2]), torch.tensor([1, 1], dtype=torch.int32), val[:2], (2, 3, 4), col, u, v)
    with pytest.raises(TypeError, match="unsupported"):
        f(crow, idx, val.to(torch.complex64), (2, 3, 4), col, u, v)
    with pytest.raises(ValueError, match="4096"):
        f(torch.zeros(3, dtype=torch.int64), idx[:0], val[:0], (1, 2, 4097), col[:1, :2], u[:1, :2],
          torch.zeros((1, 4097), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        f(crow, idx, val, (2, 3, 4), col, u, v[:, :3])
    with pytest.raises(ValueError, match="shape"):
        f(crow, idx, val, (2, 3, 4), col[:, :2], u, v)
    with pytest.raises(TypeError, match="duals"):
        f(crow, idx, val, (2, 3, 4), col, u.float(), v.float())
    with pytest.raises(TypeError, match="duals"):
        f(crow, idx, val.float(), (2, 3, 4), col, u.long(), v.long())
    with pytest.raises(TypeError, match="integer"):
        f(crow, idx, val, (2, 3, 4), col.float(), u, v)
    with pytest.raises(ValueError, match="transpose"):
        f(crow, idx, val, (2, 3, 4), col, u, v, shapes=[[3, 4], [3, 2]])
    A = torch.sparse_csr_tensor(crow, idx, val, size=(6, 4))
    with pytest.raises(ValueError, match="no batch of shape"):
        f(A, None, None, (2, 3, 5), col, u, torch.zeros((2, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):  # the sparse tensor in place of the triple reaches the state checks
        f(A, None, None, (2, 3, 4), col, u, v[:, :3])


def test_resolve_batched_sparse_of_an_empty_batch(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    for shape in ((0, 3, 4), (2, 0, 4), (0, 0, 0)):
        B, NR, NC = shape
        for dt in (torch.float64, torch.float32, torch.int32):
            col, cost, u, v, kept = lsap.resolve_batched_sparse(
                torch.zeros(B * NR + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                torch.zeros(0, dtype=dt), shape, torch.zeros((B, NR), dtype=torch.int64),
                torch.zeros((B, NR), dtype=torch.float64), torch.zeros((B, NC), dtype=torch.float64))
            assert tuple(col.shape) == (B, NR) and col.dtype == torch.int32 and bool((col == -1).all())
            assert tuple(cost.shape) == (B,) and cost.dtype == torch.float64
            assert tuple(u.shape) == (B, NR) and tuple(v.shape) == (B, NC)
            assert u.dtype == torch.float64 and v.dtype == torch.float64
            assert tuple(kept.shape) == (B,) and kept.dtype == torch.int32 and not kept.any()


def test_single_matrix_front_end_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.linear_sum_assignment_sparse_resolve
    A = (np.array([0, 1, 2, 3]), np.array([0, 1, 2], dtype=np.int32), np.ones(3), (3, 4))
    col, u, v = np.zeros(3, dtype=np.int64), np.zeros(3), np.zeros(4)
    with pytest.raises(ValueError, match="shape"):
        f(A, col, u, v[:3])
    with pytest.raises(ValueError, match="shape"):
        f(A, col[:2], u, v)
    with pytest.raises(TypeError, match="integer"):
        f(A, col.astype(np.float64), u, v)
    with pytest.raises(TypeError, match="float64"):
        f(A, col, u.astype(np.int64), v.astype(np.int64))
    with pytest.raises(TypeError, match="float64"):
        f(A, col, u.astype(np.float32), v)
    with pytest.raises(ValueError, match="4096"):
        f((np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (2, 4097)), col[:2], u[:2],
          np.zeros(4097))
    with pytest.raises(ValueError, match="sparse_csr"):
        f(torch.zeros((3, 4)), col, u, v)
    z = f((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (0, 4)),
          np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(4))
    assert [a.size for a in z] == [0, 0, 0, 4] and z[2].dtype == np.float64


# --------------------------------------------------------------------------- the expectations are not vacuous
CASES = WS.cases()
KINDS = ("partly_kept", "cascade", "infeasible_in_continuation", "infeasible_in_prologue")


def _cost(D, col):
    return D[np.arange(D.shape[0]), col].sum()


@pytest.fixture(scope="module")
def survey():
    """Per case and instance: the kind(s) the reference's warm run shows."""
    seen = {k: [] for k in KINDS}
    for family, nr, nc in CASES:
        b, w = S.batch(family, nr, nc), WS.perturbed(family, nr, nc)
        for k, (D0, D) in enumerate(zip(b.dense, w.batch.dense)):
            r, c = D.shape
            if r == 0:
                continue
            col0, v0 = w.col0[k, :r], w.v0[k, :c]
            tag = (family, nr, nc, k)
            if b.feasible[k]:  # the unperturbed instance: a fixed point
                col, _, _, kept, searches = W.warm(D0, col0, v0)
                assert kept == r and searches == 0 and np.array_equal(col, col0), tag
            try:
                c4r, r4c, u, v, kept = W.prologue(D, col0, v0)
            except ValueError:
                assert not np.isfinite(D).any(axis=1).all(), tag  # (some row has no edge)
                seen["infeasible_in_prologue"].append(tag)
                continue
            try:
                col, _, _, searches = W.replay_from(D, c4r, r4c, u, v)
            except ValueError:
                with pytest.raises(ValueError):
                    oracle.lsap(D)
                if w.changed[k] is not None:  # (else the source instance had no matching either: hall)
                    seen["infeasible_in_continuation"].append(tag)
                continue
            assert searches == r - kept, tag
            assert np.array_equal(np.sort(col), np.unique(col)) and (col >= 0).all(), tag
            assert _cost(D, col) == _cost(D, oracle.lsap(D)[1]), tag  # (the cold solve's optimum)
            if r == c and w.changed[k] is not None:
                assert kept >= r - 4, tag
            if 0 < kept < r:
                seen["partly_kept"].append(tag)
            if r < c and kept < r - 4:
                seen["cascade"].append(tag)
    return seen


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_of_instance_occurs(survey, kind):
    assert survey[kind], f"no {kind} instance over the case list"


def test_the_removed_entry_makes_bidiagonal_instances_infeasible_in_the_continuation(survey):
    """A square bidiagonal instance has one perfect matching, so the removed
    chosen entry ends it unless the added entry happens to repair it."""
    got = [t for t in survey["infeasible_in_continuation"] if t[:3] == ("bidiagonal", 64, 64)]
    assert len(got) >= 4, got


def test_perturbed_batches_are_canonical_and_differ_from_their_source():
    for family, nr, nc in CASES:
        b, w = S.batch(family, nr, nc), WS.perturbed(family, nr, nc)
        B = len(b.dense)
        lsap.validate_csr(torch.from_numpy(w.batch.indptr), torch.from_numpy(w.batch.indices),
                          torch.from_numpy(w.batch.data), (B, nr, nc),
                          None if b.corners is None else WS.shapes_of(b, nr, nc))
        for k in range(B):
            live = b.feasible[k] and b.dense[k].shape[0] >= 4
            assert (w.changed[k] is not None) == live
            if live:
                ia, ib, ic, idd = w.changed[k]
                rows = [i for i in (ia, ib, ic, idd) if i >= 0]
                assert len(set(rows)) == len(rows) and ia >= 0 and ic >= 0
                j = int(w.col0[k, ic])
                assert np.isfinite(b.dense[k][ic, j]) and w.batch.dense[k][ic, j] == np.inf
                assert np.array_equal(np.flatnonzero((b.dense[k] != w.batch.dense[k]).any(axis=1)), sorted(rows))
            else:
                assert np.array_equal(b.dense[k], w.batch.dense[k])
