"""Rectangular / ragged batched LSAP on the CPU (no GPU calls).

* the fixture tests/golden/lsap_rect_cases.npz (scipy's answers) equals the
  CPU oracle, wide and tall, ties and +inf included;
* the lsap_solve_batched_rect_* entries are declared, bound and exported, and
  their host-side argument checks answer before any device call;
* the front end's host-only pieces: the tall-result inversion and ordering,
  the `shapes` validation and the int64/float64 routing bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from conftest import load_npz_cases
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions

RECT = ("lsap_solve_batched_rect_i64", "lsap_solve_batched_rect_i32", "lsap_solve_batched_rect_f64",
        "lsap_solve_batched_rect_hash")


@pytest.fixture(scope="module")
def rect_cases():
    return load_npz_cases("lsap_rect_cases.npz")


def case_matrix(z, m):
    C = z[f"C{m['i']}"]
    return C.astype(np.int64) if m["kind"] == "int" else C.astype(np.float64)


def test_fixture_covers_the_issue_shapes(rect_cases):
    _, meta = rect_cases
    shapes = {(m["nr"], m["nc"]) for m in meta}
    for s in [(1, 1), (1, 5), (5, 1), (3, 64), (63, 65), (64, 65), (65, 64), (2, 1024), (100, 300), (300, 100)]:
        kinds = {(m["kind"].split("-")[0], m.get("hi")) for m in meta if (m["nr"], m["nc"]) == s}
        assert {("int", 3), ("int", 1 << 16), ("f64", None)} <= kinds, s
    assert shapes and sum(not m["feasible"] for m in meta) == 2
    assert sum(m["maximize"] for m in meta) == 2
    assert {"f64-ties", "f64-inf"} <= {m["kind"] for m in meta}


def test_fixture_equals_oracle(rect_cases):
    z, meta = rect_cases
    for m in meta:
        C = case_matrix(z, m)
        if m["maximize"]:
            C = -C
        if not m["feasible"]:
            with pytest.raises(ValueError):
                oracle.lsap(C)
            continue
        r, c = oracle.lsap(C)
        assert np.array_equal(r, z[f"row{m['i']}"]) and np.array_equal(c, z[f"col{m['i']}"]), m


def test_rect_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    for name in RECT:
        assert name in names and name in _lib.SIGNATURES and hasattr(L, name)


def _rect(name, nr, nc, B, C=1, col=1, modulus=7):
    """Call a rect entry with dummy non-null pointers (never dereferenced: every
    case here is answered by the host-side checks)."""
    L = _lib.lib()
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731
    if name.endswith("hash"):
        return L.lsap_solve_batched_rect_hash(ctypes.c_uint64(1), ctypes.c_int64(modulus), nr, nc, B,
                                              p(col), None, 1, None)
    return getattr(L, name)(p(C), nr, nc, B, None, p(col), None, 1, None)


@pytest.mark.parametrize("name", RECT)
def test_rect_host_checks_without_gpu(name):
    E = _lib.SH_ERR_ARGS
    assert _rect(name, 0, 5, 1) == E           # nr < 1
    assert _rect(name, -1, 5, 1) == E
    assert _rect(name, 6, 5, 1) == E           # nr > nc: tall is the caller's transpose
    assert "transpose" in _lib.last_error()
    assert _rect(name, 5, _lib.SH_MAX_N + 1, 1) == E
    assert _rect(name, 3, 5, -1) == E          # B < 0
    assert _rect(name, 3, 5, 1, col=0) == E    # null col
    if name.endswith("hash"):
        assert _rect(name, 3, 5, 1, modulus=0) == E
        assert _rect(name, 3, 5, 1, modulus=-3) == E
    else:
        assert _rect(name, 3, 5, 1, C=0) == E  # null C
    assert _rect(name, 3, 5, 0) == _lib.SH_OK  # B == 0: a no-op
    assert _rect(name, 3, 5, 0, C=0, col=0) == _lib.SH_OK
    assert _rect(name, 1024, 1024, 0) == _lib.SH_OK


def test_tall_result_is_scipys_ordering(rect_cases):
    """The transposed solve's columns are the tall matrix's rows: sorted, with
    their columns, they are scipy's (row_ind, col_ind); scattered per row they
    are solve_batched's col with -1 in the rows scipy leaves out."""
    z, meta = rect_cases
    seen = 0
    for m in meta:
        if m["nr"] <= m["nc"] or not m["feasible"]:
            continue
        seen += 1
        row, col = z[f"row{m['i']}"].astype(np.int64), z[f"col{m['i']}"].astype(np.int64)
        col_t = np.empty(m["nc"], dtype=np.int64)  # the wide solve of C.T
        col_t[col] = row
        r, c = lsap.tall_result(col_t)
        assert r.dtype == np.int64 and c.dtype == np.int64
        assert np.array_equal(r, row) and np.array_equal(c, col)
        inv = lsap.invert_tall(torch.from_numpy(np.stack([col_t, col_t]).astype(np.int32)), m["nr"])
        assert inv.dtype == torch.int32 and tuple(inv.shape) == (2, m["nr"])
        want = -np.ones(m["nr"], dtype=np.int64)
        want[row] = col
        assert np.array_equal(inv[0].numpy(), want) and np.array_equal(inv[1].numpy(), want)
    assert seen >= 8
    # an infeasible instance stays -1 everywhere
    inv = lsap.invert_tall(torch.tensor([[-1, -1, -1], [4, 0, 2]], dtype=torch.int32), 5)
    assert inv.tolist() == [[-1] * 5, [1, -1, 2, -1, 0]]


def test_shapes_validation():
    ok = lsap.check_shapes([[0, 0], [1, 1], [64, 130], [64, 64], [17, 65], [3, 129]], 6, 64, 130)
    assert ok.dtype == np.int32 and ok.shape == (6, 2) and ok.flags.c_contiguous
    assert np.array_equal(lsap.check_shapes(torch.tensor([[2, 3]], dtype=torch.int64), 1, 4, 4), [[2, 3]])
    with pytest.raises(ValueError, match="transpose"):  # a tall instance
        lsap.check_shapes([[3, 4], [5, 4]], 2, 8, 8)
    with pytest.raises(ValueError, match=r"shapes\[1\].*outside"):
        lsap.check_shapes([[3, 4], [9, 9]], 2, 8, 9)   # nr_b > NR
    with pytest.raises(ValueError, match="outside"):
        lsap.check_shapes([[3, 10]], 1, 8, 9)          # nc_b > NC
    with pytest.raises(ValueError, match="outside"):
        lsap.check_shapes([[-1, 4]], 1, 8, 9)
    with pytest.raises(ValueError, match=r"\[B, 2\]"):
        lsap.check_shapes([[3, 4]], 2, 8, 9)           # wrong B
    with pytest.raises(ValueError, match=r"\[B, 2\]"):
        lsap.check_shapes([[3.0, 4.0]], 1, 8, 9)       # not integers


def test_routing_bound_uses_the_longer_side():
    """4 (max(nr, nc) + 1) max|C| < 2^53 decides int64 against the float64
    replay: a value that passes for a 2 x 2 matrix fails for 2 x 1024 and for
    its transpose."""
    v = (1 << 53) // (4 * 3) - 1           # the largest |C| a 2 x 2 matrix may hold
    assert lsap.exact_int64_route(np.full((2, 2), v, dtype=np.int64))
    assert not lsap.exact_int64_route(np.full((2, 2), v + 2, dtype=np.int64))
    assert not lsap.exact_int64_route(np.full((2, 1024), v, dtype=np.int64))
    assert not lsap.exact_int64_route(np.full((1024, 2), v, dtype=np.int64))
    w = (1 << 53) // (4 * 1025) - 1
    assert lsap.exact_int64_route(np.full((2, 1024), -w, dtype=np.int64))
    assert lsap.exact_int64_route(np.full((1024, 2), w, dtype=np.int64))
    assert not lsap.exact_int64_route(np.full((2, 1024), -(w + 2), dtype=np.int64))
    assert not lsap.exact_int64_route(np.zeros((2, 3)))  # float input: the float64 replay
    assert lsap.exact_int64_route(np.array([[np.iinfo(np.int64).min]])) is False


def test_front_end_shape_surface_without_gpu(monkeypatch, rect_cases):
    """linear_sum_assignment's host side on wide and tall input with the
    solver stubbed by the oracle: the wide solve it hands down, the returned
    ordering, the empty and the over-size cases."""
    z, meta = rect_cases
    seen = []

    def fake(C, with_cost=True, flags=0):
        seen.append(tuple(C.shape))
        B, nr, nc = C.shape
        assert nr <= nc
        try:
            _, col = oracle.lsap(C[0].numpy())
        except ValueError:
            col = -np.ones(nr, dtype=np.int64)
        return torch.from_numpy(col.astype(np.int32)).unsqueeze(0), None

    monkeypatch.setattr(lsap, "solve_batched", fake)
    for m in meta:
        C = case_matrix(z, m)
        if not m["feasible"]:
            with pytest.raises(ValueError, match="infeasible"):
                lsap.linear_sum_assignment(C, maximize=m["maximize"], device="cpu")
            continue
        r, c = lsap.linear_sum_assignment(C, maximize=m["maximize"], device="cpu")
        assert r.dtype == np.int64 and c.dtype == np.int64
        assert np.array_equal(r, z[f"row{m['i']}"]) and np.array_equal(c, z[f"col{m['i']}"]), m
        assert seen[-1] == (1, min(m["nr"], m["nc"]), max(m["nr"], m["nc"]))
    for shape in ((0, 0), (0, 5), (5, 0)):
        r, c = lsap.linear_sum_assignment(np.zeros(shape), device="cpu")
        assert r.dtype == np.int64 and c.dtype == np.int64 and r.size == 0 and c.size == 0
    for shape in ((2, 1025), (1025, 2)):
        with pytest.raises(ValueError, match="1024"):
            lsap.linear_sum_assignment(np.zeros(shape), device="cpu")
