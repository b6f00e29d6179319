"""Free rows on the CSR on the CPU (no GPU calls): the reference
of tests/free_rows_ref.py on the densifications of
tests/free_rows_sparse_families.py, the new entries' declarations and host
checks, the front ends' argument errors and empty batches, and the new kernels'
names and resources.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import free_rows_ref as FR
import free_rows_sparse_families as F
import lsap_duals_ref as R
import lsap_warm_ref as W
from santa_hip import _lib, lsap
from test_cabi_cpu import HEADER, declared_functions
from test_kernel_resources_cpu import _kernel_meta

SUFFIXES = ("f64", "f32")
PREFIX = "fcsr_"
# a new kernel's mangled name may contain none of these: existing tests count kernels by them
COUNTED = ("lsap_", "lbap", "murty_", "kbest_", "warm_csr_", "mcsr_", "frow_", "bneck_")


# --------------------------------------------------------------------------- the families and the reference
def test_family_is_canonical_and_holds_what_it_promises():
    names = {g.name: g for g in F.family()}
    for g in F.family():
        nr, nc = g.shape
        assert g.indptr[0] == 0 and g.indptr[-1] == g.indices.size == g.data.size and len(g.indptr) == nr + 1
        for i in range(nr):
            row = g.indices[g.indptr[i]:g.indptr[i + 1]]
            assert (np.diff(row) > 0).all() and ((row >= 0) & (row < nc)).all()
    P = {k: np.isfinite(names[k].dense) for k in ("empty_word_mid", "empty_word_last", "many_virtual", "all_and_none")}
    assert not P["empty_word_mid"][:, 64:128].any() and P["empty_word_mid"][:, :64].any()
    assert P["empty_word_mid"][:, 128:].any() and np.flatnonzero(P["empty_word_mid"][0]).min() >= 128
    assert not P["empty_word_last"][:, 128:].any()
    assert 150 - 20 > 64 and 300 - 30 > 256 and names["many_virtual"].shape == (30, 300)
    assert names["one_row"].shape[0] == 1
    assert P["all_and_none"][:, 2].all() and not P["all_and_none"][:, 5].any()
    assert (names["all_and_none"].data == 0).any() and np.isinf(names["all_and_none"].data).any()
    assert not F.feasible(names["hall_wide"]) and not F.feasible(names["hall"]) and not F.feasible(names["empty_row"])
    assert names["hall"].shape[0] < names["hall"].shape[1]   # wide: the virtual rows have every column
    assert any(g.corner != g.shape and g.corner[0] > 0 for g in F.family())
    kinds = {s[0] for g in F.family() for s in F.states(g)}
    assert kinds == {"solved", "dropped", "garbage", "empty"}


def _brute(D):
    nr, nc = D.shape
    return min(D[np.arange(nr), list(p)].sum() for p in itertools.permutations(range(nc), nr))


def test_reference_on_the_densifications_is_the_padded_warm_start_and_optimal():
    brute = 0
    for g in F.family():
        D = np.asarray(g.dense)
        nr, nc = D.shape
        if nr == 0:
            continue
        for name, col0, v0 in F.states(g):
            col0, v0 = col0[:nr].astype(np.int64), v0[:nc]
            if not F.feasible(g):
                with pytest.raises(ValueError, match="infeasible"):
                    FR.resolve(D, col0, v0)
                continue
            P, c4r, r4c, su, sv, kept, kept_free = FR.start_state(D, col0, v0)
            r = FR.resolve(D, col0, v0)
            pc, pu, pv, pkept, psearches = W.warm(P, c4r, v0)   # the written-out padded matrix
            assert pkept == kept + kept_free and psearches == r.searches, (g.name, name)
            assert np.array_equal(pc[:nr], r.col) and np.array_equal(pu[:nr], r.u) and np.array_equal(pv, r.v)
            assert r.theta == pv.max()
            assert np.isfinite(D[np.arange(nr), r.col]).all()
            assert r.cost == D[np.arange(nr), R.replay(D)[0]].sum(), (g.name, name)
            if name == "solved":
                assert r.searches == 0 and r.kept == nr and r.kept_free == nc - nr, g.name
            if name == "dropped":
                # the row loses its pair; where it names another row's column from below, that row loses its claim too
                assert r.kept in (nr - 1, nr - 2), g.name
            if nc <= 7 and name == "empty":
                assert r.cost == _brute(D), g.name
                brute += 1
    assert brute > 20


@pytest.mark.parametrize("nr,nc", ((57, 64), (120, 128)))
def test_k_redrawn_rows_of_a_sparse_instance_cost_at_most_k_searches(nr, nc):
    rng = np.random.default_rng([nr, nc, 23])
    P = rng.random((nr, nc)) < 0.3
    P[np.arange(nr), np.arange(nr)] = True
    D = np.where(P, rng.integers(0, 1 << 16, size=(nr, nc)).astype(np.float64), np.inf)
    col, _, v = R.replay(D)
    for k in (1, 3):
        E = D.copy()
        rows = rng.choice(nr, size=k, replace=False)
        E[rows] = np.where(P[rows], rng.integers(0, 1 << 16, size=(k, nc)).astype(np.float64), np.inf)
        r = FR.resolve(E, col, v)
        assert r.kept >= nr - k and r.kept_free == nc - nr and r.searches <= k
        assert r.cost == E[np.arange(nr), R.replay(E)[0]].sum()


# --------------------------------------------------------------------------- the C-ABI
def test_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    header = " ".join(open(HEADER).read().split())

    def decl(name):
        d = header[header.index(f"int {name}("):]
        return d[:d.index(";")]

    for suf in SUFFIXES:
        name = f"lsap_warm_fr_csr_{suf}"
        assert name in names and hasattr(L, name), name
        # indptr, indices, data, nr, nc, B, shape, col, cost, u, v, kept, theta, work, work_bytes, flags, stream
        assert _lib.SIGNATURES[name] == (I, [P, P, P, I, I, I, P, P, P, P, P, P, P, P, Z, U, P]), name
        d = decl(name)
        assert d.count(",") == 16
        assert "int32_t *d_kept, double *d_theta, void *d_work, size_t work_bytes, unsigned flags, void *stream" in d
        # lsap_warm_csr_'s list with d_theta put in after d_kept
        assert d.replace("lsap_warm_fr_csr_", "lsap_warm_csr_").replace(" double *d_theta,", "") == \
            decl(f"lsap_warm_csr_{suf}"), suf
        for stem in ("lsap_murty_children_", "lsap_kbest_"):
            name, sib = f"{stem}fr_csr_{suf}", f"{stem}csr_{suf}"
            assert name in names and hasattr(L, name), name
            assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sib]
            assert decl(name).replace(name, sib) == decl(sib), name
    import santa_hip
    assert hasattr(santa_hip, "resolve_batched_sparse_free_rows")
    assert "resolve_batched_sparse_free_rows" in santa_hip.__all__


def _p(x):
    return ctypes.c_void_p(x) if x else None  # (never dereferenced)


def _warm(suf, nr, nc, B, work=0x1000, work_bytes=None, indices=0x1000, data=0x1000, kept=0, theta=0, **null):
    a = {k: 0x1000 for k in ("indptr", "col", "u", "v")}
    a.update(null)
    if work_bytes is None:
        work_bytes = _lib.lib().lsap_csr_work_bytes(nr, nc, B)
    return getattr(_lib.lib(), "lsap_warm_fr_csr_" + suf)(
        _p(a["indptr"]), _p(indices), _p(data), nr, nc, B, None, _p(a["col"]), None, _p(a["u"]), _p(a["v"]), _p(kept),
        _p(theta), _p(work), work_bytes, 0, None)


def _children(suf, nr, nc, B, work=0x1000, work_bytes=1 << 40, indices=0x1000, data=0x1000, **null):
    a = {k: 0x1000 for k in ("indptr", "pcol", "pv", "p", "forb", "col", "cost", "u", "v")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_murty_children_fr_csr_" + suf)(
        _p(a["indptr"]), _p(indices), _p(data), nr, nc, B, None, _p(a["pcol"]), _p(a["pv"]), _p(a["p"]),
        _p(a["forb"]), _p(a["col"]), _p(a["cost"]), _p(a["u"]), _p(a["v"]), None, _p(work), work_bytes, 0, None)


def _kbest(suf, nr, nc, B, k, work=0x1000, work_bytes=1 << 40, flags=0, indices=0x1000, data=0x1000, **null):
    a = {k_: 0x1000 for k_ in ("indptr", "cols", "costs", "count")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_kbest_fr_csr_" + suf)(
        _p(a["indptr"]), _p(indices), _p(data), nr, nc, B, None, k, _p(a["cols"]), _p(a["costs"]), _p(a["count"]),
        _p(work), work_bytes, flags, None)


@pytest.mark.parametrize("suf", SUFFIXES)
def test_warm_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    assert _warm(suf, 0, 5, 1) == E
    assert _warm(suf, 6, 5, 1) == E
    assert "transpose" in _lib.last_error()
    assert _warm(suf, 5, _lib.SH_MAX_N_LARGE + 1, 1) == E
    assert "4096" in _lib.last_error()
    assert _warm(suf, 3, 5, -1) == E
    for null in ("indptr", "col", "u", "v"):
        assert _warm(suf, 3, 5, 1, **{null: 0}) == E, null
    need = _lib.lib().lsap_csr_work_bytes(3, 5, 2)
    assert need > 0
    assert _warm(suf, 3, 5, 2, work_bytes=need - 1) == E
    assert "lsap_csr_work_bytes" in _lib.last_error()
    assert _warm(suf, 3, 5, 2, work=0) == E
    assert _warm(suf, 3, 5, 2, work=0x1004) == E
    assert "aligned" in _lib.last_error()
    B = (1 << 31) // 1024 * 4 + 8   # B * nr too large for the grid of the pass over the CSR
    assert _warm(suf, 1024, 1024, B, work_bytes=1 << 62) == E
    assert "too large" in _lib.last_error()
    # B == 0 is a no-op after the checks, with or without the nullable outputs
    assert _warm(suf, 3, 5, 0) == _lib.SH_OK
    assert _warm(suf, 3, 5, 0, kept=0x1000, theta=0x1000) == _lib.SH_OK
    assert _warm(suf, 3, 5, 0, indptr=0, col=0, u=0, v=0, work=0, indices=0, data=0) == _lib.SH_OK
    assert _warm(suf, 4096, 4096, 0) == _lib.SH_OK and _warm(suf, 1, 4096, 0) == _lib.SH_OK
    assert _warm(suf, 6, 5, 0) == E


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
    need = _lib.lib().lsap_kbest_csr_work_bytes(3, 5, 2, 4)   # (the pool of lsap_kbest_csr_, unchanged)
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


# --------------------------------------------------------------------------- the code object
def test_new_kernels_are_the_two_launch_tables_without_scratch(tmp_path):
    meta = _kernel_meta(tmp_path)
    new = {k: v for k, v in meta.items() if PREFIX in k}
    assert not [(k, s) for k in new for s in COUNTED if s in k], "a new kernel's name contains a counted substring"
    assert not {k: v for k, v in new.items() if v}, "kernels with private (scratch) memory"
    want = set()
    for s in "df":
        # launch_warm_csr's table: one wave up to 64 columns; four waves, 10-bit keys, 1 / 2 / 4 columns a thread up
        # to 1024; with_large_f64_cfg beyond
        want.add(f"fcsr_prep_kernelI{s}E")
        want.add(f"fcsr_kernelILi1E{s}E")
        want |= {f"fcsr_mw_kernelILi{nw}ELi{k}E{s}Li{fb}EE"
                 for nw, k, fb in ((4, 1, 10), (4, 2, 10), (4, 4, 10), (8, 4, 12), (8, 6, 12), (8, 8, 12))}
    assert len(want) == 16
    for s in "df":
        # launch_mcsr's table, up to 1024 columns
        want.add(f"fcsr_mprep_kernelI{s}E")
        want.add(f"fcsr_mf64_kernelILi1E{s}E")
        want |= {f"fcsr_mf64_mw_kernelILi4ELi{k}E{s}Li10EE" for k in (1, 2, 4)}
    assert len(want) == 26
    for w in want:
        assert sum(w in k for k in new) == 1, w
    assert len(new) == 26


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


def test_resolve_batched_sparse_free_rows_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.resolve_batched_sparse_free_rows
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
    with pytest.raises(TypeError, match="integer"):
        f(crow, idx, val, (2, 3, 4), col.float(), u, v)
    with pytest.raises(ValueError, match="transpose"):
        f(crow, idx, val, (2, 3, 4), col, u, v, shapes=[[3, 4], [3, 2]])
    A = torch.sparse_csr_tensor(crow, idx, val, size=(6, 4))
    with pytest.raises(ValueError, match="no batch of shape"):
        f(A, None, None, (2, 3, 5), col, u, torch.zeros((2, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):  # the sparse tensor in place of the triple reaches the state checks
        f(A, None, None, (2, 3, 4), col, u, v[:, :3])


def test_the_free_rows_switches_check_their_arguments_before_the_device(no_gpu):
    crow, idx, val = _triple()
    with pytest.raises(ValueError, match="k must be"):
        lsap.kbest_batched_sparse(crow, idx, val, (2, 3, 4), k=0, free_rows=True)
    with pytest.raises(ValueError, match="1024"):
        lsap.kbest_batched_sparse(torch.zeros(3, dtype=torch.int64), idx[:0], val[:0], (1, 2, 1025), k=2,
                                  free_rows=True)
    A = torch.sparse_csr_tensor(crow, idx, val, size=(6, 4))
    with pytest.raises(ValueError, match="k must be"):
        lsap.kbest_batched_sparse(A, shape=(2, 3, 4), k=0, free_rows=True)
    col, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.float64)
    p, forb = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ValueError, match="expected col"):
        lsap.murty_children_batched_sparse(crow, idx, val, (2, 3, 4), col[:, :2], v, p, forb, free_rows=True)
    with pytest.raises(TypeError, match="float64"):
        lsap.murty_children_batched_sparse(crow, idx, val, (2, 3, 4), col, v.float(), p, forb, free_rows=True)
    M = (np.array([0, 1, 2, 3]), np.array([0, 1, 2], dtype=np.int32), np.ones(3), (3, 4))
    with pytest.raises(ValueError, match="k must be"):
        lsap.kbest_assignments_sparse(M, 0, free_rows=True)
    with pytest.raises(ValueError, match="1024"):
        lsap.kbest_assignments_sparse((np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0),
                                       (2, 1025)), 2, free_rows=True)
    cols, costs = lsap.kbest_assignments_sparse((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                                 np.zeros(0), (0, 4)), 2, free_rows=True)
    assert cols.shape == (0, 0) and costs.shape == (0,)
    g = lsap.linear_sum_assignment_sparse_resolve
    c3, u3, v4 = np.zeros(3, dtype=np.int64), np.zeros(3), np.zeros(4)
    with pytest.raises(ValueError, match="shape"):
        g(M, c3, u3, v4[:3], free_rows=True)
    with pytest.raises(TypeError, match="float64"):
        g(M, c3, u3.astype(np.float32), v4, free_rows=True)
    z = g((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (0, 4)),
          np.zeros(0, dtype=np.int64), np.zeros(0), v4, free_rows=True)
    assert [a.size for a in z] == [0, 0, 0, 4]


def test_empty_batches(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    inf = float("inf")
    for shape in ((0, 3, 4), (2, 0, 4), (0, 0, 0)):
        B, NR, NC = shape
        crow, idx = torch.zeros(B * NR + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
        for dt in (torch.float64, torch.float32):
            val = torch.zeros(0, dtype=dt)
            col, cost, u, v, kept, kept_free, theta = lsap.resolve_batched_sparse_free_rows(
                crow, idx, val, shape, torch.zeros((B, NR), dtype=torch.int64),
                torch.zeros((B, NR), dtype=torch.float64), torch.zeros((B, NC), dtype=torch.float64))
            assert tuple(col.shape) == (B, NR) and col.dtype == torch.int32 and bool((col == -1).all())
            assert tuple(cost.shape) == (B,) and cost.dtype == torch.float64
            assert tuple(u.shape) == (B, NR) and tuple(v.shape) == (B, NC)
            for k in (kept, kept_free):
                assert tuple(k.shape) == (B,) and k.dtype == torch.int32 and not k.any()
            assert tuple(theta.shape) == (B,) and theta.dtype == torch.float64 and not theta.any()
            cols, costs, count = lsap.kbest_batched_sparse(crow, idx, val, shape, k=5, free_rows=True)
            assert tuple(cols.shape) == (B, 5, NR) and bool((cols == -1).all())
            assert tuple(costs.shape) == (B, 5) and bool((costs == inf).all()) and not count.any()
            ccol, ccost, cu, cv, ckept = lsap.murty_children_batched_sparse(
                crow, idx, val, shape, torch.zeros((B, NR), dtype=torch.int32), torch.zeros((B, NC), dtype=torch.float64),
                torch.zeros(B, dtype=torch.int32), torch.zeros((B, (NC + 63) // 64), dtype=torch.int64),
                free_rows=True)
            assert tuple(ccol.shape) == (B, NR, NR) and bool((ccol == -1).all()) and bool((ccost == inf).all())
            assert tuple(cu.shape) == (B, NR, NR) and tuple(cv.shape) == (B, NR, NC) and not ckept.any()
