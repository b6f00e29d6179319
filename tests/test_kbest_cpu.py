"""The k best assignments on the CPU (no GPU calls): the reference of
tests/kbest_ref.py proved against brute force, the lsap_murty_children_ and
lsap_kbest_ entries' declarations and host checks, and the Python front ends'
argument errors and empty-batch answers.
"""
import ctypes

import numpy as np
import pytest
import torch

import kbest_families as KF
import kbest_ref as KR
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions

SUFFIXES = ("f64", "f32")


# --------------------------------------------------------------------------- the reference
def test_reference_against_brute_force():
    short = infeasible = square_children = 0
    for C in KF.small_family():
        nr, nc = C.shape
        want = KF.brute_force(C)
        cols, costs, count, searches, trace = KR.kbest(C, KF.K_SMALL)
        assert len(trace) == count and (count == 0 or trace[0] is None)
        assert count == min(KF.K_SMALL, want.size), C
        assert np.array_equal(costs[:count], want[:count]), C
        KF.check_assignments(C, cols, costs, count)
        if nr == nc:
            assert all(s == 1 for s in searches), (C, searches)
            square_children += len(searches)
        short += 0 < count < KF.K_SMALL
        infeasible += count == 0
    assert short and infeasible and square_children


def test_reference_order_of_ties_and_k_one():
    C = np.zeros((3, 3))  # every assignment costs 0: the order is the creation order
    cols, costs, count, _, _ = KR.kbest(C, 6)
    assert count == 6 and (costs == 0).all()
    assert cols[0].tolist() == KR.replay(C)[0].tolist()
    assert len({tuple(c) for c in cols.tolist()}) == 6
    one = KR.kbest(KF.small_family()[0], 1)
    assert one[2] == 1 and one[3] == []  # the last rank is not expanded


def test_tail_sum_is_a_sum():
    x = np.arange(1.0, 200.0)
    assert KR.tail_sum(x) == x.sum() and KR.tail_sum([]) == 0.0 and KR.tail_sum([np.inf, 1.0]) == np.inf


def test_masked_matrix_is_the_definition():
    C = np.arange(20.0).reshape(4, 5)
    col = np.array([1, 0, 3, 4])
    F = np.zeros(5, dtype=bool)
    F[2] = True
    Ft = KR.forbidden_t(col, 2, F, 2)
    assert Ft.tolist() == [False, False, True, True, False]
    assert KR.forbidden_t(col, 1, F, 2).tolist() == [False, False, False, True, False]  # t > p: F is dropped
    M = KR.masked(C, col, 2, Ft)
    inf = np.inf
    assert M.tolist() == [[inf, 1, inf, inf, inf], [5, inf, inf, inf, inf], [inf, inf, inf, inf, 14],
                          [inf, inf, 17, 18, 19]]


# --------------------------------------------------------------------------- the C-ABI
def test_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
    for suf in SUFFIXES:
        for name in (f"lsap_murty_children_{suf}", f"lsap_kbest_{suf}"):
            assert name in names and hasattr(L, name), name
        assert _lib.SIGNATURES[f"lsap_murty_children_{suf}"] == (I, [P, I, I, I, P, P, P, P, P, P, P, P, P, P, U, P])
        assert _lib.SIGNATURES[f"lsap_kbest_{suf}"] == (I, [P, I, I, I, P, I, P, P, P, P, Z, U, P])
    assert "lsap_kbest_work_bytes" in names and _lib.SIGNATURES["lsap_kbest_work_bytes"] == (Z, [I, I, I, I])
    import santa_hip
    for name in ("kbest_batched", "kbest_assignments", "murty_children_batched"):
        assert hasattr(santa_hip, name) and name in santa_hip.__all__, name


def _p(x):
    return ctypes.c_void_p(x) if x else None  # (never dereferenced)


def _children(suf, nr, nc, B, **null):
    a = {k: 0x1000 for k in ("C", "pcol", "pv", "p", "forb", "col", "cost", "u", "v")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_murty_children_" + suf)(
        _p(a["C"]), nr, nc, B, None, _p(a["pcol"]), _p(a["pv"]), _p(a["p"]), _p(a["forb"]), _p(a["col"]),
        _p(a["cost"]), _p(a["u"]), _p(a["v"]), None, 0, None)


def _kbest(suf, nr, nc, B, k, work=0x1000, work_bytes=1 << 40, **null):
    a = {k_: 0x1000 for k_ in ("C", "cols", "costs", "count")}
    a.update(null)
    return getattr(_lib.lib(), "lsap_kbest_" + suf)(
        _p(a["C"]), nr, nc, B, None, k, _p(a["cols"]), _p(a["costs"]), _p(a["count"]), _p(work), work_bytes, 0, None)


@pytest.mark.parametrize("suf", SUFFIXES)
def test_children_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    assert _children(suf, 0, 5, 1) == E
    assert _children(suf, 6, 5, 1) == E
    assert "transpose" in _lib.last_error()
    assert _children(suf, 5, _lib.SH_MAX_N + 1, 1) == E
    assert "1024" in _lib.last_error()
    assert _children(suf, 3, 5, -1) == E
    for null in ("C", "pcol", "pv", "p", "forb", "col", "cost", "u", "v"):
        assert _children(suf, 3, 5, 1, **{null: 0}) == E, null
    assert _children(suf, 3, 5, 0) == _lib.SH_OK
    assert _children(suf, 1024, 1024, 0, C=0, pcol=0, pv=0, p=0, forb=0, col=0, cost=0, u=0, v=0) == _lib.SH_OK


@pytest.mark.parametrize("suf", SUFFIXES)
def test_kbest_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    need = _lib.lib().lsap_kbest_work_bytes(3, 5, 2, 4)
    assert need > 0 and need % 8 == 0
    assert _kbest(suf, 0, 5, 1, 4) == E
    assert _kbest(suf, 6, 5, 1, 4) == E
    assert _kbest(suf, 5, _lib.SH_MAX_N + 1, 1, 4) == E
    assert _kbest(suf, 3, 5, -1, 4) == E
    assert _kbest(suf, 3, 5, 2, 0) == E
    assert "k < 1" in _lib.last_error()
    for null in ("C", "cols", "costs", "count"):
        assert _kbest(suf, 3, 5, 2, 4, **{null: 0}) == E, null
    assert _kbest(suf, 3, 5, 2, 4, work=0) == E
    assert _kbest(suf, 3, 5, 2, 4, work_bytes=need - 1) == E
    assert "work_bytes" in _lib.last_error()
    assert _kbest(suf, 3, 5, 2, 4, work=0x1004, work_bytes=need) == E
    assert "aligned" in _lib.last_error()
    assert _kbest(suf, 3, 5, 0, 4, work=0x1004, work_bytes=0) == E  # (the alignment is checked for B == 0 too)
    assert _kbest(suf, 3, 5, 0, 4) == _lib.SH_OK
    assert _kbest(suf, 3, 5, 0, 4, work=0, work_bytes=0, C=0, cols=0, costs=0, count=0) == _lib.SH_OK


def test_work_bytes_is_monotone_in_k_and_zero_on_rejected_arguments():
    f = _lib.lib().lsap_kbest_work_bytes
    for nr, nc, B in ((1, 1, 1), (3, 5, 2), (64, 64, 7), (250, 257, 3), (1024, 1024, 1)):
        sizes = [f(nr, nc, B, k) for k in (1, 2, 3, 10, 100)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (nr, nc, B, sizes)
        W = (nc + 63) // 64
        # what the pool holds for every node: col, v, F and cost (the total is rounded up to 8 bytes)
        assert abs(sizes[2] - sizes[1] - B * nr * (4 * nr + 8 * nc + 8 * W + 8)) <= 4, (nr, nc, B)
    for bad in ((0, 5, 1, 3), (6, 5, 1, 3), (5, 1025, 1, 3), (3, 5, -1, 3), (3, 5, 1, 0), (3, 5, 1, -2)):
        assert f(*bad) == 0, bad
    assert f(1024, 1024, 1 << 20, 1 << 30) == 0  # (does not fit a size_t: rejected, not wrapped)


# --------------------------------------------------------------------------- the front ends
@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise AssertionError("a host check should have answered first")
    monkeypatch.setattr(lsap, "require_gpu", refuse)


@pytest.mark.parametrize("dtype", (torch.int64, torch.int32, torch.float16, torch.bfloat16))
def test_kbest_refuses_integer_and_16_bit_costs(no_gpu, dtype):
    C = torch.zeros((2, 3, 4), dtype=dtype)
    with pytest.raises(TypeError, match="float64 or float32.*no forbidden value"):
        lsap.kbest_batched(C, 3)
    with pytest.raises(TypeError, match="float64 or float32.*no forbidden value"):
        lsap.murty_children_batched(C, torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.float64),
                                    torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64))


def test_kbest_batched_checks_its_arguments_before_the_device(no_gpu):
    C = torch.zeros((2, 3, 4), dtype=torch.float64)
    for k in (0, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            lsap.kbest_batched(C, k)
    with pytest.raises(ValueError, match=r"\[B, NR, NC\]"):
        lsap.kbest_batched(C[0], 2)
    with pytest.raises(ValueError, match="1024"):
        lsap.kbest_batched(torch.zeros((1, 2, 1025)), 2)
    with pytest.raises(ValueError, match="padded wide"):
        lsap.kbest_batched(C.transpose(1, 2), 2, shapes=[[3, 3], [3, 3]])
    with pytest.raises(ValueError, match="k must be"):
        lsap.kbest_assignments(np.zeros((3, 3)), 0)
    with pytest.raises(ValueError, match="matrix"):
        lsap.kbest_assignments(np.zeros(3), 2)
    with pytest.raises(ValueError, match="invalid numeric"):
        lsap.kbest_assignments(np.array([[0.0, np.nan]]), 2)
    with pytest.raises(ValueError, match="invalid numeric"):
        lsap.kbest_assignments(np.array([[0.0, np.inf]]), 2, maximize=True)
    with pytest.raises(ValueError, match="1024"):
        lsap.kbest_assignments(np.zeros((2, 1025)), 2)
    cols, costs = lsap.kbest_assignments(np.zeros((0, 4)), 3)
    assert cols.shape == (0, 0) and costs.shape == (0,)


def test_murty_children_batched_checks_its_arguments_before_the_device(no_gpu):
    C = torch.zeros((2, 3, 4), dtype=torch.float32)
    col, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.float64)
    p, forb = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ValueError, match="expected col"):
        lsap.murty_children_batched(C, col[:, :2], v, p, forb)
    with pytest.raises(ValueError, match="expected col"):
        lsap.murty_children_batched(C, col, v, p, torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(TypeError, match="float64"):
        lsap.murty_children_batched(C, col, v.float(), p, forb)
    with pytest.raises(TypeError, match="int64"):
        lsap.murty_children_batched(C, col, v, p, forb.to(torch.int32))
    with pytest.raises(TypeError, match="integer"):
        lsap.murty_children_batched(C, col.double(), v, p, forb)
    with pytest.raises(ValueError, match="wide or square"):
        lsap.murty_children_batched(C.transpose(1, 2), col, v, p, forb)


def test_empty_batches(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    inf = float("inf")
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        B, NR, NC = shape
        for maximize in (False, True):
            cols, costs, count = lsap.kbest_batched(torch.zeros(shape, dtype=torch.float32), 5, maximize=maximize)
            assert tuple(cols.shape) == (B, 5, NR) and cols.dtype == torch.int32 and bool((cols == -1).all())
            assert tuple(costs.shape) == (B, 5) and costs.dtype == torch.float64
            assert bool((costs == (-inf if maximize else inf)).all())
            assert tuple(count.shape) == (B,) and count.dtype == torch.int32 and not count.any()
    for shape in ((0, 3, 4), (2, 0, 4)):
        B, NR, NC = shape
        col, cost, u, v, kept = lsap.murty_children_batched(
            torch.zeros(shape, dtype=torch.float64), torch.zeros((B, NR), dtype=torch.int32),
            torch.zeros((B, NC), dtype=torch.float64), torch.zeros(B, dtype=torch.int32),
            torch.zeros((B, (NC + 63) // 64), dtype=torch.int64))
        assert tuple(col.shape) == (B, NR, NR) and bool((col == -1).all())
        assert tuple(cost.shape) == (B, NR) and bool((cost == inf).all())
        assert tuple(u.shape) == (B, NR, NR) and tuple(v.shape) == (B, NR, NC) and tuple(kept.shape) == (B, NR)
