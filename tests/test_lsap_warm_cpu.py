"""The warm start of the batched LSAP solver on the CPU (no GPU calls): the
reference of tests/lsap_warm_ref.py proved against the cold replay, the
lsap_warm_ entries' declarations and host checks, and the Python front ends'
argument errors.

* prologue(C, *replay(C)) is the identity with kept == nr;
* from a perturbed or a garbage state the warm result satisfies the four exact
  invariants of integer duals, costs what the cold replay costs, and runs
  nr - kept searches;
* one changed entry of a square instance drops at most one pair;
* the raise loop's result does not depend on the order of its pops;
* the window's edges: -2^56 is a dual, -2^56 - 1 is not.
"""
import ctypes

import numpy as np
import pytest
import torch

import lsap_duals_ref as R
import lsap_families as F
import lsap_warm_ref as W
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
WARM = tuple(f"lsap_warm_{t}" for t in SUFFIXES)
OK = {"feasible": True, "tight": True, "sign": True, "gap": True}
# integer families whose replays stay quick; square and wide
SHAPES = ((24, 24), (33, 40), (40, 40), (17, 64))
FAMILIES = ("mw", "mw_neg", "mw_ties", "two_scale42", "neg_cols", "window_edges", "i32_extremes")
CASES = [(f, nr, nc) for f in FAMILIES for nr, nc in SHAPES]
IDS = [f"{f}-{nr}x{nc}" for f, nr, nc in CASES]


def cost_of(C, col):
    return int(np.asarray(C).astype(object)[np.arange(len(col)), col].sum())


def random_cases(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        nc = int(rng.integers(2, 40))
        nr = nc if rng.random() < 0.5 else int(rng.integers(1, nc + 1))
        hi = int(rng.choice([3, 50, 100000]))
        yield rng, rng.integers(-hi, hi, size=(nr, nc), dtype=np.int64)


def check_warm(C, col0, v0):
    col, u, v, kept, searches = W.warm(C, col0, v0)
    nr = C.shape[0]
    assert searches == nr - kept
    assert np.array_equal(np.sort(col), np.unique(col)) and (col >= 0).all()
    assert R.invariants(C, col, u, v) == OK
    assert cost_of(C, col) == cost_of(C, R.replay(C)[0])
    return kept


@pytest.mark.parametrize("family,nr,nc", CASES, ids=IDS)
def test_prologue_of_a_solution_is_the_identity(family, nr, nc):
    C = F.make(family, "int64", nr, nc)
    col, u, v = R.replay(C)
    c4r, r4c, pu, pv, kept = W.prologue(C, col, v)
    assert kept == nr
    assert np.array_equal(c4r, col) and np.array_equal(pu, u) and np.array_equal(pv, v)
    inv = -np.ones(nc, dtype=np.int64)
    inv[col] = np.arange(nr)
    assert np.array_equal(r4c, inv)
    wc, wu, wv, searches = W.replay_from(C, c4r, r4c, pu, pv)
    assert searches == 0 and np.array_equal(wc, col) and np.array_equal(wu, u) and np.array_equal(wv, v)


@pytest.mark.parametrize("family,nr,nc", CASES, ids=IDS)
def test_perturbed_entries_matched_ones_included(family, nr, nc):
    C = F.make(family, "int64", nr, nc)
    col, u, v = R.replay(C)
    rng = np.random.default_rng([7, nr, nc, len(family)])
    span = max(1, int(np.abs(C).max()) // 4)
    for k in (1, 2, 3):
        D = C.copy()
        rows = rng.choice(nr, size=min(k, nr), replace=False)
        for t, i in enumerate(rows):
            j = int(col[i]) if t == 0 else int(rng.integers(0, nc))  # (the first hit is a matched entry)
            D[i, j] += int(rng.integers(-span, span + 1))
        kept = check_warm(D, col, v)
        assert kept >= nr - len(rows) if nr == nc else kept >= 0


def test_random_instances_from_perturbed_and_garbage_states():
    for rng, C in random_cases(20261020, 120):
        nr, nc = C.shape
        col, u, v = R.replay(C)
        D = C.copy()
        for _ in range(int(rng.integers(1, 4))):
            D[rng.integers(0, nr), rng.integers(0, nc)] += int(rng.integers(-50, 51))
        check_warm(D, col, v)
        # garbage: columns out of range and duplicated, duals positive or far below the window
        col0 = rng.integers(-5, nc + 5, size=nr)
        v0 = rng.integers(-60, 20, size=nc).astype(np.int64)
        v0[rng.random(nc) < 0.2] = -(1 << 60)
        check_warm(D, col0, v0)
        check_warm(D, -np.ones(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64))  # the empty state: a cold run


def test_empty_state_is_the_cold_replay():
    C = F.make("mw", "int64", 20, 24)
    col, u, v = R.replay(C)
    wc, wu, wv, kept, searches = W.warm(C, -np.ones(20, dtype=np.int64), np.zeros(24, dtype=np.int64))
    # u starts at the row minima instead of 0, so the run differs from the cold one; its optimum does not
    assert kept == 0 and searches == 20 and cost_of(C, wc) == cost_of(C, col)
    assert R.invariants(C, wc, wu, wv) == OK


@pytest.mark.parametrize("n", (5, 24, 40))
def test_one_changed_entry_of_a_square_instance_drops_at_most_one_pair(n):
    rng = np.random.default_rng(n)
    C = rng.integers(0, 100, size=(n, n), dtype=np.int64)
    col, u, v = R.replay(C)
    for i in range(n):
        for j in (int(col[i]), int(rng.integers(0, n))):
            for d in (-7, 9):
                D = C.copy()
                D[i, j] += d
                assert W.prologue(D, col, v)[4] >= n - 1


def test_the_raise_loop_does_not_depend_on_the_order_of_its_pops():
    seen_cascade = False
    for rng, C in random_cases(99, 150):
        nr, nc = C.shape
        if nr == nc:
            continue
        col, u, v = R.replay(C)
        D = C.copy()
        for _ in range(3):
            D[rng.integers(0, nr), rng.integers(0, nc)] -= int(rng.integers(1, 60))
        a = W.prologue(D, col, v, order="fifo")
        b = W.prologue(D, col, v, order="lifo")
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        seen_cascade |= a[4] < nr - 3  # more pairs lost than entries changed: the raise loop cascaded
    assert seen_cascade


def test_window_edges_of_the_previous_duals():
    C = np.full((3, 3), 5, dtype=np.int64)
    v0 = np.array([-(1 << 56), -(1 << 56) - 1, 3], dtype=np.int64)
    assert W.sanitise(v0, np.int64).tolist() == [-(1 << 56), 0, 0]
    c4r, _, u, v, kept = W.prologue(C, np.array([0, 1, 2]), v0)
    # (square: nothing is raised, the dual stays; its pair is not tight and goes)
    assert v.tolist() == [-(1 << 56), 0, 0] and u.tolist() == [5, 5, 5] and c4r.tolist() == [-1, 1, 2] and kept == 2
    assert check_warm(C, np.array([0, 1, 2]), v0) == 2
    f = np.array([-1.5, np.nan, -np.inf, np.inf, 2.0, -0.0])
    assert W.sanitise(f, np.float64).tolist() == [-1.5, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_float_prologue_reports_an_all_inf_row():
    C = np.ones((3, 4))
    C[1] = np.inf
    with pytest.raises(ValueError, match="infeasible"):
        W.prologue(C, [0, 1, 2], np.zeros(4))
    C = np.ones((3, 3))
    C[:, 0] = np.inf  # no row can take column 0: only the continuation sees it
    c4r, r4c, u, v, _ = W.prologue(C, [0, 1, 2], np.zeros(3))
    with pytest.raises(ValueError, match="infeasible"):
        W.replay_from(C, c4r, r4c, u, v)


def test_float_warm_equals_value_of_cold():
    rng = np.random.default_rng(5)
    C = rng.integers(0, 64, size=(30, 37)).astype(np.float64)
    col, u, v = R.replay(C)
    D = C.copy()
    D[3, col[3]] += 11.0
    D[8, 2] = 0.0
    wc, wu, wv, kept, searches = W.warm(D, col, v)
    assert searches == 30 - kept and D[np.arange(30), wc].sum() == D[np.arange(30), R.replay(D)[0]].sum()
    assert R.invariants(D.astype(np.int64), wc, wu.astype(np.int64), wv.astype(np.int64)) == OK


# --------------------------------------------------------------------------- the C-ABI
def test_warm_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    for name in WARM:
        assert name in names and hasattr(L, name), name
        # C, nr, nc, B, shape, col, cost, u, v, kept, flags, stream -- the header's list
        assert _lib.SIGNATURES[name] == (I, [P, I, I, I, P, P, P, P, P, P, U, P]), name
    header = open(__import__("test_cabi_cpu").HEADER).read()
    for suf in SUFFIXES:
        decl = header[header.index(f"int lsap_warm_{suf}("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") == 11 and "int32_t *d_kept, unsigned flags, void *stream" in " ".join(decl.split()), suf
    import santa_hip
    for name in ("resolve_batched", "linear_sum_assignment_resolve"):
        assert hasattr(santa_hip, name) and name in santa_hip.__all__, name


def _call(name, nr, nc, B, C=1, col=1, u=1, v=1):
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731  (never dereferenced)
    return getattr(_lib.lib(), name)(p(C), nr, nc, B, None, p(col), None, p(u), p(v), None, 0, None)


@pytest.mark.parametrize("name", WARM)
def test_warm_host_checks_without_gpu(name):
    E = _lib.SH_ERR_ARGS
    assert _call(name, 0, 5, 1) == E
    assert _call(name, 6, 5, 1) == E
    assert "transpose" in _lib.last_error()
    assert _call(name, 5, _lib.SH_MAX_N_LARGE + 1, 1) == E
    assert "4096" in _lib.last_error()
    assert _call(name, 3, 5, -1) == E
    for null in ("C", "col", "u", "v"):
        assert _call(name, 3, 5, 1, **{null: 0}) == E, null
    assert _call(name, 3, 5, 0) == _lib.SH_OK
    assert _call(name, 3, 5, 0, C=0, col=0, u=0, v=0) == _lib.SH_OK
    assert _call(name, 4096, 4096, 0) == _lib.SH_OK


# --------------------------------------------------------------------------- the front ends
@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise AssertionError("a host check should have answered first")
    monkeypatch.setattr(lsap, "require_gpu", refuse)


def test_resolve_batched_checks_its_arguments_before_the_device(no_gpu):
    C = torch.zeros((2, 3, 4), dtype=torch.int64)
    col = torch.zeros((2, 3), dtype=torch.int32)
    u, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, NR, NC\]"):
        lsap.resolve_batched(C[0], col, u, v)
    with pytest.raises(ValueError, match="shape"):
        lsap.resolve_batched(C, col, u, v[:, :3])
    with pytest.raises(ValueError, match="shape"):
        lsap.resolve_batched(C, col[:, :2], u, v)
    with pytest.raises(TypeError, match="duals"):
        lsap.resolve_batched(C, col, u.double(), v.double())
    with pytest.raises(TypeError, match="duals"):
        lsap.resolve_batched(C.float(), col, u, v)
    with pytest.raises(TypeError, match="integer"):
        lsap.resolve_batched(C, col.float(), u, v)
    with pytest.raises(TypeError, match="unsupported"):
        lsap.resolve_batched(C.to(torch.int16), col, u, v)
    with pytest.raises(ValueError, match="4096"):
        lsap.resolve_batched(torch.zeros((1, 2, 4097), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32),
                             torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 4097), dtype=torch.int64))
    with pytest.raises(ValueError, match="transpose"):
        lsap.resolve_batched(C, col, u, v, shapes=[[3, 4], [3, 2]])
    with pytest.raises(ValueError, match="padded wide"):
        lsap.resolve_batched(C.transpose(1, 2), torch.zeros((2, 4), dtype=torch.int32), v, u, shapes=[[3, 3], [3, 3]])


def test_resolve_batched_of_an_empty_batch(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        B, NR, NC = shape
        for dt, ddt in ((torch.int32, torch.int64), (torch.float16, torch.float64)):
            col, cost, u, v, kept = lsap.resolve_batched(
                torch.zeros(shape, dtype=dt), torch.zeros((B, NR), dtype=torch.int64),
                torch.zeros((B, NR), dtype=ddt), torch.zeros((B, NC), dtype=ddt))
            assert tuple(col.shape) == (B, NR) and col.dtype == torch.int32 and bool((col == -1).all())
            assert tuple(cost.shape) == (B,) and cost.dtype == ddt
            assert tuple(u.shape) == (B, NR) and tuple(v.shape) == (B, NC) and u.dtype == ddt and v.dtype == ddt
            assert tuple(kept.shape) == (B,) and kept.dtype == torch.int32 and not kept.any()


def test_single_matrix_front_end_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.linear_sum_assignment_resolve
    C = np.arange(12).reshape(3, 4)
    col, u, v = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="matrix"):
        f(C[0], col, u, v)
    with pytest.raises(ValueError, match="shape"):
        f(C, col, u, v[:3])
    with pytest.raises(ValueError, match="shape"):
        f(C.T, col, u, v)  # (tall: col_ind and u have one entry per row)
    with pytest.raises(TypeError, match="integer"):
        f(C, col.astype(np.float64), u, v)
    with pytest.raises(TypeError, match="int64"):  # the exact integer route wants int64 duals
        f(C, col, u.astype(np.float64), v.astype(np.float64))
    with pytest.raises(TypeError, match="float64"):  # a float matrix: the float64 route
        f(C + 0.5, col, u, v)
    with pytest.raises(TypeError, match="float64"):  # integers too wide for the exact route
        f(C.astype(np.int64) << 52, col, u, v)
    with pytest.raises(ValueError, match="invalid numeric"):
        f(np.where(C == 5, np.nan, C + 0.5), col, u.astype(np.float64), v.astype(np.float64))
    with pytest.raises(ValueError, match="4096"):
        f(np.zeros((2, 4097)), col[:2], np.zeros(2), np.zeros(4097))
    z = f(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(4, dtype=np.int64))
    assert [a.size for a in z] == [0, 0, 0, 4]
