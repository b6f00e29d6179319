"""Dual variables of the batched LSAP solvers on the CPU (no GPU calls).

* the replay helpers of lsap_duals_ref.py: the vectorised form equals the
  scalar loop bit for bit, both reproduce the oracle's and scipy's columns, and
  integer duals satisfy the four invariants exactly;
* the lsap_solve_batched_duals_* and lsap_check_duals_* entries are declared,
  bound and exported, and their host-side argument checks answer before any
  device call;
* the front end's host-only pieces: the default return value, the inversion of
  a tall col for the certificate, the exported names.
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import lsap_duals_ref as R
import lsap_families as F
import oracle
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions

try:  # (scipy itself where it is installed; the oracle replays it everywhere)
    from scipy.optimize import linear_sum_assignment as scipy_lsa
except ImportError:
    scipy_lsa = None

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
SOLVE = tuple(f"lsap_solve_batched_duals_{t}" for t in SUFFIXES)
CHECK = tuple(f"lsap_check_duals_{t}" for t in SUFFIXES)


def float_cases():
    rng = np.random.default_rng(20251019)
    cases = [(f"random-{nr}x{nc}", rng.random((nr, nc))) for nr, nc in ((40, 40), (63, 65), (100, 257))]
    cases.append(("ties-63x65", rng.integers(0, 3, size=(63, 65)) * 0.5))
    C = rng.random((40, 48))
    C[rng.random((40, 48)) < 0.3] = np.inf
    C[np.arange(40), np.arange(40)] = rng.random(40)  # (a finite diagonal keeps it feasible)
    cases.append(("inf-40x48", C))
    return cases


FLOAT_CASES = float_cases()
INT_CASES = [(f, nr, nc) for f in F.INT_FAMILIES for nr, nc in ((63, 64), (65, 65))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name,C", FLOAT_CASES, ids=[n for n, _ in FLOAT_CASES])
def test_float_replay_vectorised_equals_scalar_bit_for_bit(name, C):
    col, u, v = R.replay(C)
    cs, us, vs = R.replay_scalar(C)
    assert u.dtype == np.float64 and v.dtype == np.float64
    assert np.array_equal(col, cs)
    assert np.array_equal(bits(u), bits(us)) and np.array_equal(bits(v), bits(vs))
    r, c = oracle.lsap(C)
    assert np.array_equal(r, np.arange(C.shape[0])) and np.array_equal(col, c)
    if scipy_lsa is not None:
        assert np.array_equal(col, scipy_lsa(C)[1])


def test_float_replay_reports_infeasible():
    C = np.ones((3, 4))
    C[1] = np.inf
    for f in (R.replay, R.replay_scalar):
        with pytest.raises(ValueError, match="infeasible"):
            f(C)


@pytest.mark.parametrize("family,nr,nc", INT_CASES, ids=[f"{f}-{nr}x{nc}" for f, nr, nc in INT_CASES])
def test_integer_replay_columns_and_invariants(family, nr, nc):
    C = F.make(family, "int64", nr, nc)
    col, u, v = R.replay(C)
    assert u.dtype == np.int64 and v.dtype == np.int64
    assert np.array_equal(col, oracle.lsap(C)[1])
    if scipy_lsa is not None:
        assert np.array_equal(col, scipy_lsa(C)[1])
    assert R.invariants(C, col, u, v) == {"feasible": True, "tight": True, "sign": True, "gap": True}


@pytest.mark.parametrize("seed,nr,nc,lo,hi", [(1, 5, 5, -4, 5), (2, 40, 40, 0, 3), (3, 30, 100, -1000, 1000),
                                              (4, 12, 12, 0, 2)])
def test_integer_replay_scalar_cross_check(seed, nr, nc, lo, hi):
    C = np.random.default_rng(seed).integers(lo, hi, size=(nr, nc), dtype=np.int64)
    col, u, v = R.replay(C)
    cs, us, vs = R.replay_scalar(C)
    assert np.array_equal(col, cs) and np.array_equal(u, us) and np.array_equal(v, vs)
    assert all(R.invariants(C, col, u, v).values())


# --------------------------------------------------------------------------- the C-ABI
def test_duals_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    for name in SOLVE + CHECK:
        assert name in names and name in _lib.SIGNATURES and hasattr(L, name), name
    import santa_hip
    for name in ("check_duals", "linear_sum_assignment_duals", "SH_CERT_COL", "SH_CERT_SLACK", "SH_CERT_TIGHT",
                 "SH_CERT_SIGN", "SH_CERT_GAP", "SH_CERT_NONE", "SH_CERT_RANGE"):
        assert hasattr(santa_hip, name) and name in santa_hip.__all__, name
    assert [santa_hip.SH_CERT_COL, santa_hip.SH_CERT_SLACK, santa_hip.SH_CERT_TIGHT, santa_hip.SH_CERT_SIGN,
            santa_hip.SH_CERT_GAP, santa_hip.SH_CERT_NONE, santa_hip.SH_CERT_RANGE] == [1, 2, 4, 8, 16, 32, 64]
    header = open(__import__("test_cabi_cpu").HEADER).read()
    for name, value in (("COL", 1), ("SLACK", 2), ("TIGHT", 4), ("SIGN", 8), ("GAP", 16), ("NONE", 32), ("RANGE", 64)):
        assert f"#define SH_CERT_{name} {value} " in header
    assert L.sh_version() == 1


def _call(name, nr, nc, B, C=1, col=1, u=1, v=1, flags=1):
    """Call a duals entry with dummy non-null pointers (never dereferenced:
    every case here is answered by the host-side checks)."""
    L = _lib.lib()
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731
    if name in SOLVE:
        return getattr(L, name)(p(C), nr, nc, B, None, p(col), None, p(u), p(v), flags, None)
    return getattr(L, name)(p(C), nr, nc, B, None, p(col), p(u), p(v), p(1), p(1), None)


@pytest.mark.parametrize("name", SOLVE + CHECK)
def test_duals_host_checks_without_gpu(name):
    E = _lib.SH_ERR_ARGS
    assert _call(name, 0, 5, 1) == E           # nr < 1
    assert _call(name, -1, 5, 1) == E
    assert _call(name, 6, 5, 1) == E           # nr > nc: tall is the caller's transpose
    assert "transpose" in _lib.last_error()
    assert _call(name, 5, _lib.SH_MAX_N + 1, 1) == E
    assert "1024" in _lib.last_error()
    assert _call(name, 3, 5, -1) == E          # B < 0
    assert _call(name, 3, 5, 1, C=0) == E      # null C
    assert _call(name, 3, 5, 1, col=0) == E    # null col
    assert _call(name, 3, 5, 1, u=0) == E      # null u
    assert _call(name, 3, 5, 1, v=0) == E      # null v
    assert _call(name, 3, 5, 0) == _lib.SH_OK  # B == 0: a no-op
    assert _call(name, 3, 5, 0, C=0, col=0, u=0, v=0) == _lib.SH_OK
    assert _call(name, 1024, 1024, 0) == _lib.SH_OK


@pytest.mark.parametrize("name", SOLVE[2:])
def test_float_duals_entries_refuse_both_designs(name):
    both = _lib.SH_FLAG_F64_MW | _lib.SH_FLAG_F64_SW
    assert _call(name, 3, 5, 1, flags=both) == _lib.SH_ERR_ARGS
    assert "exclude" in _lib.last_error()
    assert _call(name, 3, 5, 0, flags=both) == _lib.SH_ERR_ARGS  # (as the _rect_ entries: before B == 0)


def test_check_entry_refuses_null_outputs():
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    for name in CHECK:
        assert getattr(L, name)(p, 3, 5, 1, None, p, p, p, None, p, None) == _lib.SH_ERR_ARGS  # null slack
        assert getattr(L, name)(p, 3, 5, 1, None, p, p, p, p, None, None) == _lib.SH_ERR_ARGS  # null flags


# --------------------------------------------------------------------------- the front end
@pytest.fixture
def no_gpu_needed(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)


@pytest.mark.parametrize("shape", [(0, 3, 4), (2, 0, 4), (2, 3, 0), (0, 0, 0)])
def test_solve_batched_default_is_a_pair_and_empty_duals_are_zeros(no_gpu_needed, shape):
    assert inspect.signature(lsap.solve_batched).parameters["duals"].default is False
    B, NR, NC = shape
    for dt, ddt in ((torch.int64, torch.int64), (torch.int32, torch.int64), (torch.float32, torch.float64),
                    (torch.bfloat16, torch.float64)):
        out = lsap.solve_batched(torch.zeros(shape, dtype=dt))
        assert isinstance(out, tuple) and len(out) == 2
        col, cost, u, v = lsap.solve_batched(torch.zeros(shape, dtype=dt), duals=True)
        assert tuple(col.shape) == (B, NR) and col.dtype == torch.int32 and bool((col == -1).all())
        assert tuple(cost.shape) == (B,) and cost.dtype == ddt
        assert tuple(u.shape) == (B, NR) and tuple(v.shape) == (B, NC) and u.dtype == ddt and v.dtype == ddt
        assert not u.any() and not v.any()
        res = lsap.check_duals(torch.zeros(shape, dtype=dt), col, u, v)
        assert [tuple(t.shape) for t in res] == [(B,)] * 4
        assert res[0].dtype == ddt and res[3].dtype == torch.int32 and not res[3].any()


def test_check_duals_validates_its_arguments(no_gpu_needed):
    C = torch.zeros((2, 3, 4), dtype=torch.int64)
    col = torch.zeros((2, 3), dtype=torch.int32)
    u, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, NR, NC\]"):
        lsap.check_duals(C[0], col, u, v)
    with pytest.raises(ValueError, match="shape"):
        lsap.check_duals(C, col, u, v[:, :3])
    with pytest.raises(TypeError, match="duals"):
        lsap.check_duals(C, col, u.double(), v.double())
    with pytest.raises(TypeError, match="unsupported"):
        lsap.check_duals(C.to(torch.int16), col, u, v)
    with pytest.raises(ValueError, match="transpose"):  # check_shapes: a tall instance
        lsap.check_duals(C, col, u, v, shapes=[[3, 4], [3, 2]])
    with pytest.raises(ValueError, match="padded wide"):
        lsap.check_duals(C.transpose(1, 2), torch.zeros((2, 4), dtype=torch.int32), v, u, shapes=[[3, 3], [3, 3]])
    with pytest.raises(ValueError, match="1024"):
        lsap.check_duals(torch.zeros((1, 2, 1025), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32),
                         torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 1025), dtype=torch.int64))


def test_invert_col_is_the_tall_certificates_inverse():
    """A tall batch is certified as its transpose: col [B, NR] (columns of the
    rows scipy kept, -1 elsewhere) becomes the transposed solve's per-row
    columns [B, NC]; a col that is no assignment is reported, not inverted."""
    col_t = torch.tensor([[4, 0, 2], [1, 2, 3]], dtype=torch.int32)  # the wide solve of a 5 x 3 batch
    col = lsap.invert_tall(col_t, 5)
    inv, bad = lsap.invert_col(col, 3)
    assert inv.dtype == torch.int32 and torch.equal(inv, col_t) and bad.tolist() == [False, False]
    inv, bad = lsap.invert_col(torch.tensor([[1, -1, 2, -1, -1],     # column 0 left free: fine here,
                                             [1, -1, 1, -1, 0],      # a column taken twice
                                             [3, -1, 1, -1, 0],      # a column outside [0, 3)
                                             [-2, -1, 1, 2, 0],      # below -1
                                             [-1, -1, -1, -1, -1]], dtype=torch.int32), 3)
    assert bad.tolist() == [False, True, True, True, False]
    assert inv[0].tolist() == [-1, 0, 2] and inv[4].tolist() == [-1, -1, -1]


def test_recorded_replays_are_current_and_certified():
    """tests/golden/lsap_duals_replay.npz (the replays too long to repeat in
    every run): each matrix still hashes to what was recorded, the columns are
    the oracle's, integer duals pass the exact certificate and float duals are
    tight and feasible to within an ulp of the entries."""
    for key in R.RECORDED:
        family, dtype, nr, nc, k = key
        C = F.instance(*key)
        col, u, v = R.replay_instance(*key)  # (asserts the sha)
        assert col.shape == (nr,) and u.shape == (nr,) and v.shape == (nc,) and u.dtype == C.dtype
        assert np.array_equal(col, oracle.lsap(C)[1]), key
        S = C - u[:, None] - v[None, :]
        free = np.ones(nc, dtype=bool)
        free[col] = False
        assert (v <= 0).all() and not v[free].any(), key
        if dtype == "int64":
            assert (S >= 0).all() and not S[np.arange(nr), col].any(), key
            assert int(u.sum()) + int(v.sum()) == int(C[np.arange(nr), col].sum()), key
        else:
            tol = 8 * np.finfo(np.float64).eps * np.abs(C).max()
            assert S.min() >= -tol and np.abs(S[np.arange(nr), col]).max() <= tol, key
