"""The free-rows warm start on the CPU (no GPU calls): the
reference of tests/free_rows_ref.py proved against the existing definitions
applied to the written-out padded matrix, the lsap_warm_fr_ entries'
declarations and host checks, the front ends' argument errors, and the new
kernels' resources.

* the reference's start state is lsap_warm_ref.prologue's of the padded matrix
  (asserted inside free_rows_ref.start_state on every call made here) and its
  result lsap_warm_ref.warm's;
* from solved, perturbed, garbage and empty states the result is a valid
  assignment at the cold replay's cost, with (nr - kept) + (nc - nr -
  kept_free) searches;
* from a solver state with k redrawn rows exactly the redrawn rows can lose
  their pair and every virtual row keeps one: at most k searches, where the
  existing warm start runs a cascade;
* integer duals come back normalised: the four exact invariants of
  lsap_duals_ref.invariants on the unpadded matrix, and a fixed point when fed
  back.
"""
import ctypes

import numpy as np
import pytest
import torch

import free_rows_ref as FR
import lsap_duals_ref as R
import lsap_warm_ref as W
from santa_hip import _lib, lsap
from test_cabi_cpu import HEADER, declared_functions
from test_kernel_resources_cpu import _kernel_meta

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
ENTRIES = tuple(f"lsap_warm_fr_{t}" for t in SUFFIXES)
OK = {"feasible": True, "tight": True, "sign": True, "gap": True}
# a new kernel's mangled name may contain none of these: existing resource tests count kernels by them
FORBIDDEN = ("lsap_", "murty_", "kbest_", "mcsr_", "warm_csr_", "lbap", "bneck_")


def cost_of(C, col):
    return int(np.asarray(C).astype(object)[np.arange(len(col)), col].sum())


def random_cases(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        nc = int(rng.integers(2, 40))
        nr = nc if rng.random() < 0.25 else int(rng.integers(1, nc + 1))
        hi = int(rng.choice([3, 50, 100000]))
        yield rng, rng.integers(-hi, hi, size=(nr, nc), dtype=np.int64)


def check(C, col0, v0):
    """Everything that holds from any state; -> the result."""
    nr, nc = C.shape
    r = FR.resolve(C, col0, v0)   # (asserts the equality with the padded prologue and the search count)
    assert np.array_equal(np.sort(r.col), np.unique(r.col)) and (r.col >= 0).all() and (r.col < nc).all()
    assert int(r.cost) == cost_of(C, r.col) == cost_of(C, R.replay(C)[0])
    assert R.invariants(C, r.col, r.u, r.v) == OK   # normalised: v <= 0, 0 on the free columns
    assert 0 <= r.kept <= nr and 0 <= r.kept_free <= nc - nr
    assert r.searches == (nr - r.kept) + (nc - nr - r.kept_free)
    # ... and the result is a fixed point: nothing runs from it, and nothing moves
    again = FR.resolve(C, r.col, r.v)
    assert again.searches == 0 and again.kept == nr and again.kept_free == nc - nr
    assert np.array_equal(again.col, r.col) and np.array_equal(again.u, r.u) and np.array_equal(again.v, r.v)
    assert again.theta == 0 or nr == nc
    return r


def test_reference_is_the_warm_start_of_the_written_out_padded_matrix():
    for rng, C in random_cases(1, 60):
        nr, nc = C.shape
        col, u, v = R.replay(C)
        D = C.copy()
        D[rng.integers(0, nr)] = rng.integers(-50, 50, size=nc)
        for col0, v0 in ((col, v), (rng.integers(-3, nc + 3, size=nr), rng.integers(-60, 20, size=nc))):
            P, c4r, r4c, su, sv, kept, kept_free = FR.start_state(D, col0, v0)
            r = FR.resolve(D, col0, v0)
            pc, pu, pv, pkept, psearches = W.warm(P, c4r, v0)
            assert pkept == kept + kept_free and psearches == r.searches
            assert np.array_equal(pc[:nr], r.col)
            shift = r.theta if nr < nc else 0
            assert np.array_equal(pu[:nr] + shift, r.u) and np.array_equal(pv - shift, r.v)
            assert r.theta == pv.max() and (pu[nr:] == -r.theta).all()
            # every column no real row holds ends at theta
            free = np.ones(nc, dtype=bool)
            free[r.col] = False
            assert (pv[free] == r.theta).all()


def test_float_reference_is_bit_for_bit_the_padded_warm_start():
    rng = np.random.default_rng(3)
    for nr, nc in ((9, 40), (30, 37), (40, 47), (12, 12)):
        C = rng.random((nr, nc)) * 100
        col, u, v = R.replay(C)
        D = C.copy()
        D[nr // 2] = rng.random(nc) * 100
        P, c4r, r4c, su, sv, kept, kept_free = FR.start_state(D, col, v)
        r = FR.resolve(D, col, v)
        pc, pu, pv, _, _ = W.warm(P, c4r, v)
        assert np.array_equal(pc[:nr], r.col)
        assert pu[:nr].tobytes() == r.u.tobytes() and pv.tobytes() == r.v.tobytes()   # no shift in floats
        assert r.theta == pv.max() and np.float64(r.theta).tobytes() == np.float64(0.0 - (0.0 - pv).min()).tobytes()
        assert D[np.arange(nr), r.col].sum() == pytest.approx(D[np.arange(nr), R.replay(D)[0]].sum(), rel=1e-12)


def test_random_instances_from_solved_perturbed_garbage_and_empty_states():
    for rng, C in random_cases(20261021, 100):
        nr, nc = C.shape
        col, u, v = R.replay(C)
        r = check(C, col, v)   # the solved state: nothing to do
        assert r.searches == 0 and np.array_equal(r.col, col)
        D = C.copy()
        for _ in range(int(rng.integers(1, 4))):
            D[rng.integers(0, nr), rng.integers(0, nc)] += int(rng.integers(-50, 51))
        check(D, col, v)
        col0 = rng.integers(-5, nc + 5, size=nr)
        v0 = rng.integers(-60, 20, size=nc).astype(np.int64)
        v0[rng.random(nc) < 0.2] = -(1 << 60)
        check(D, col0, v0)
        r = check(D, -np.ones(nr, dtype=np.int64), np.zeros(nc, dtype=np.int64))   # the empty state
        assert r.kept == 0 and r.kept_free == nc - nr and r.searches == nr


@pytest.mark.parametrize("nr,nc", ((57, 64), (250, 256), (16, 128)))
def test_k_redrawn_rows_cost_at_most_k_searches(nr, nc):
    rng = np.random.default_rng([nr, nc])
    C = rng.integers(0, 1 << 16, size=(nr, nc), dtype=np.int64)
    col, u, v = R.replay(C)
    for k in (1, 3):
        D = C.copy()
        rows = rng.choice(nr, size=k, replace=False)
        D[rows] = rng.integers(0, 1 << 16, size=(k, nc))
        r = FR.resolve(D, col, v)
        assert r.kept >= nr - k and r.kept_free == nc - nr and r.searches <= k
        assert int(r.cost) == cost_of(D, R.replay(D)[0]) and R.invariants(D, r.col, r.u, r.v) == OK
        # the existing warm start raises columns and cascades on the same input where nearly every column has a
        # row (with 16 rows on 128 columns most duals are 0 already and there is little to raise)
        assert 8 * nr <= nc or W.warm(D, col, v)[4] > 4 * k


def test_a_real_row_that_drops_its_pair_frees_the_column_for_a_virtual_row():
    # row 1 names column 2 and is not tight there; column 2 holds theta = 0, so virtual row 2 takes it
    C = np.array([[1, 5, 5, 5], [5, 1, 9, 5]], dtype=np.int64)
    P, c4r, r4c, u, v, kept, kept_free = FR.start_state(C, [0, 2], np.zeros(4, dtype=np.int64))
    assert kept == 1 and kept_free == 2 and c4r.tolist() == [0, -1, 1, 2] and r4c.tolist() == [0, 2, 3, -1]
    r = check(C, [0, 2], np.zeros(4, dtype=np.int64))
    assert r.col.tolist() == [0, 1] and r.searches == 1


def test_float_infeasibility_is_the_padded_problem_s():
    C = np.ones((3, 5))
    C[1] = np.inf
    with pytest.raises(ValueError, match="infeasible"):
        FR.resolve(C, [0, 1, 2], np.zeros(5))
    C = np.ones((3, 5))
    C[:2, 1:] = np.inf   # rows 0 and 1 both need column 0
    with pytest.raises(ValueError, match="infeasible"):
        FR.resolve(C, [0, 1, 2], np.zeros(5))


# --------------------------------------------------------------------------- the C-ABI
def test_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    header = open(HEADER).read()
    for suf, name in zip(SUFFIXES, ENTRIES):
        assert name in names and hasattr(L, name), name
        # C, nr, nc, B, shape, col, cost, u, v, kept, theta, flags, stream -- the header's list
        assert _lib.SIGNATURES[name] == (I, [P, I, I, I, P, P, P, P, P, P, P, U, P]), name
        decl = header[header.index(f"int {name}("):]
        decl = " ".join(decl[:decl.index(";")].split())
        assert decl.count(",") == 12, suf
        dual = "int64_t" if suf[0] == "i" else "double"
        assert f"int32_t *d_kept, {dual} *d_theta, unsigned flags, void *stream" in decl, suf
        # lsap_warm_'s list with d_theta put in
        warm = header[header.index(f"int lsap_warm_{suf}("):]
        warm = " ".join(warm[:warm.index(";")].split())
        assert decl.replace("lsap_warm_fr_", "lsap_warm_").replace(f" {dual} *d_theta,", "") == warm, suf
    import santa_hip
    assert hasattr(santa_hip, "resolve_batched_free_rows") and "resolve_batched_free_rows" in santa_hip.__all__


def _call(name, nr, nc, B, C=1, col=1, u=1, v=1):
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731  (never dereferenced)
    return getattr(_lib.lib(), name)(p(C), nr, nc, B, None, p(col), None, p(u), p(v), None, None, 0, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_host_checks_without_gpu(name):
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
    assert _call(name, 1, 4096, 0) == _lib.SH_OK


# --------------------------------------------------------------------------- the front ends
@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise AssertionError("a host check should have answered first")
    monkeypatch.setattr(lsap, "require_gpu", refuse)


def test_front_end_checks_its_arguments_before_the_device(no_gpu):
    f = lsap.resolve_batched_free_rows
    C = torch.zeros((2, 3, 4), dtype=torch.int64)
    col = torch.zeros((2, 3), dtype=torch.int32)
    u, v = torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, NR, NC\]"):
        f(C[0], col, u, v)
    with pytest.raises(ValueError, match="shape"):
        f(C, col, u, v[:, :3])
    with pytest.raises(ValueError, match="shape"):
        f(C, col[:, :2], u, v)
    with pytest.raises(TypeError, match="duals"):
        f(C, col, u.double(), v.double())
    with pytest.raises(TypeError, match="duals"):
        f(C.float(), col, u, v)
    with pytest.raises(TypeError, match="integer"):
        f(C, col.float(), u, v)
    with pytest.raises(TypeError, match="unsupported"):
        f(C.to(torch.int16), col, u, v)
    with pytest.raises(ValueError, match="4096"):
        f(torch.zeros((1, 2, 4097), dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32),
          torch.zeros((1, 2), dtype=torch.int64), torch.zeros((1, 4097), dtype=torch.int64))
    with pytest.raises(ValueError, match="transpose"):
        f(C, col, u, v, shapes=[[3, 4], [3, 2]])
    with pytest.raises(ValueError, match="padded wide"):
        f(C.transpose(1, 2), torch.zeros((2, 4), dtype=torch.int32), v, u, shapes=[[3, 3], [3, 3]])
    g = lsap.linear_sum_assignment_resolve
    M = np.arange(12).reshape(3, 4)
    z3, z4 = np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match="shape"):
        g(M, z3, z3, z4[:3], free_rows=True)
    with pytest.raises(TypeError, match="int64"):
        g(M, z3, z3.astype(np.float64), z4.astype(np.float64), free_rows=True)
    with pytest.raises(TypeError, match="float64"):
        g(M + 0.5, z3, z3, z4, free_rows=True)
    z = g(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), z4, free_rows=True)
    assert [a.size for a in z] == [0, 0, 0, 4]


def test_front_end_of_an_empty_batch(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
        B, NR, NC = shape
        for dt, ddt in ((torch.int32, torch.int64), (torch.float16, torch.float64)):
            col, cost, u, v, kept, kept_free, theta = lsap.resolve_batched_free_rows(
                torch.zeros(shape, dtype=dt), torch.zeros((B, NR), dtype=torch.int64),
                torch.zeros((B, NR), dtype=ddt), torch.zeros((B, NC), dtype=ddt))
            assert tuple(col.shape) == (B, NR) and col.dtype == torch.int32 and bool((col == -1).all())
            assert tuple(cost.shape) == (B,) and cost.dtype == ddt
            assert tuple(u.shape) == (B, NR) and tuple(v.shape) == (B, NC) and u.dtype == ddt and v.dtype == ddt
            for k in (kept, kept_free):
                assert tuple(k.shape) == (B,) and k.dtype == torch.int32 and not k.any()
            assert tuple(theta.shape) == (B,) and theta.dtype == ddt and not theta.any()


# --------------------------------------------------------------------------- the kernels
def test_new_kernels_are_the_launch_table_without_scratch(tmp_path):
    meta = _kernel_meta(tmp_path)
    new = {k: v for k, v in meta.items() if "frow_" in k}
    assert not [k for k in new for s in FORBIDDEN if s in k], "a new kernel's name contains a counted substring"
    assert not {k: v for k, v in new.items() if v}, "kernels with private (scratch) memory"
    S = {"i64": "l", "i32": "i", "f64": "d", "f32": "f", "f16": "DF16_", "bf16": "NS_7sh_bf16E"}
    want = {f"frow_prep_kernelI{S[s]}{'l' if s[0] == 'i' else 'd'}E" for s in SUFFIXES}
    # launch_warm's table: one wave up to 64 columns; four waves, 10-bit keys, 1 / 2 / 4 columns a thread up to
    # 1024; with_large_cfg / with_large_f64_cfg beyond
    for s in ("i64", "i32"):
        want |= {f"frow_i64_kernelILi{nw}ELi{k}E{S[s]}Li{fb}EE"
                 for nw, k, fb in ((1, 1, 10), (4, 1, 10), (4, 2, 10), (4, 4, 10), (8, 4, 12), (16, 3, 12), (16, 4, 12))}
    for s in ("f64", "f32", "f16", "bf16"):
        want.add(f"frow_f64_kernelILi1E{S[s]}E")
        want |= {f"frow_f64_mw_kernelILi{nw}ELi{k}E{S[s]}Li{fb}EE"
                 for nw, k, fb in ((4, 1, 10), (4, 2, 10), (4, 4, 10), (8, 4, 12), (8, 6, 12), (8, 8, 12))}
    assert len(want) == 6 + 14 + 28
    # the k-best children: launch_murty's table, float64 and float32 costs up to 1024 columns
    for s in ("f64", "f32"):
        want.add(f"frow_mprep_kernelI{S[s]}E")
        want.add(f"frow_mf64_kernelILi1E{S[s]}E")
        want |= {f"frow_mf64_mw_kernelILi4ELi{k}E{S[s]}Li10EE" for k in (1, 2, 4)}
    assert len(want) == 48 + 10
    for w in want:
        assert sum(w in k for k in new) == 1, w
    assert len(new) == len(want)


# --------------------------------------------------------------------------- Murty's partition with free rows
def test_kbest_reference_with_free_rows_children_equals_brute_force():
    import kbest_families as KF
    wide = 0
    for C in KF.small_family():
        nr, nc = C.shape
        want = KF.brute_force(C)
        cols, costs, count, searches, _ = FR.kbest(C, KF.K_SMALL)
        assert count == min(KF.K_SMALL, want.size)
        assert np.array_equal(costs[:count], want[:count])
        KF.check_assignments(C, cols, costs, count)
        wide += nr < nc
    assert wide > 10


@pytest.mark.parametrize("nr,nc", ((9, 40), (20, 23), (33, 40), (40, 47), (12, 12)))
def test_a_child_of_an_integer_valued_instance_runs_exactly_one_search(nr, nc):
    import kbest_ref as K
    rng = np.random.default_rng([nr, nc, 5])
    C = rng.integers(0, 1000, size=(nr, nc)).astype(np.float64)
    col, _, v = R.replay(C)
    F = np.zeros(nc, dtype=bool)
    node = (col, v, 0, F)
    many = 0
    for depth in range(3):   # the root, then a child of it, then a grandchild
        col, v, p, F = node
        nxt = None
        for t in range(p, nr):
            got = FR.child(C, col, v, p, F, t)
            old = K.child(C, col, v, p, F, t) if depth == 0 else None   # (the existing child of the root)
            if got is None:
                assert depth > 0 or old is None
                continue
            c, u, v2, kept, searches, Ft = got
            assert searches == 1 and kept == nr - 1, (depth, t, searches, kept)
            M = K.masked(C, col, t, Ft)
            want = M[np.arange(nr), R.replay(M)[0]].sum()
            assert C[np.arange(nr), c].sum() == want
            if old is not None:
                many = max(many, old[4])
            if t == (p + nr) // 2:
                nxt = (c, v2, t, Ft)
        if nxt is None:
            break
        node = nxt
    assert nr == nc or nc - nr > 8 or many > 1   # the existing child of a nearly square wide instance cascades


def test_kbest_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    header = " ".join(open(HEADER).read().split())
    for suf in ("f64", "f32"):
        for stem in ("lsap_murty_children_", "lsap_kbest_"):
            name, sib = f"{stem}fr_{suf}", f"{stem}{suf}"
            assert name in names and hasattr(L, name), name
            assert _lib.SIGNATURES[name] == _lib.SIGNATURES[sib]
            decl = header[header.index(f"int {name}("):]
            want = header[header.index(f"int {sib}("):]
            assert decl[:decl.index(";")].replace(name, sib) == want[:want.index(";")], name


@pytest.mark.parametrize("suf", ("f64", "f32"))
def test_kbest_host_checks_without_gpu(suf):
    E = _lib.SH_ERR_ARGS
    L = _lib.lib()
    q = ctypes.c_void_p(0x1000)   # (never dereferenced)
    ch = getattr(L, f"lsap_murty_children_fr_{suf}")
    kb = getattr(L, f"lsap_kbest_fr_{suf}")

    def children(nr, nc, B, **null):
        a = {k: (None if k in null else q) for k in ("C", "pcol", "pv", "p", "forb", "col", "cost", "u", "v")}
        return ch(a["C"], nr, nc, B, None, a["pcol"], a["pv"], a["p"], a["forb"], a["col"], a["cost"], a["u"], a["v"],
                  None, 0, None)

    def kbest(nr, nc, B, k, work=q, nbytes=None, **null):
        a = {k_: (None if k_ in null else q) for k_ in ("C", "cols", "costs", "count")}
        nbytes = int(L.lsap_kbest_work_bytes(nr, nc, B, k)) if nbytes is None else nbytes
        return kb(a["C"], nr, nc, B, None, k, a["cols"], a["costs"], a["count"], work, nbytes, 0, None)

    for call in (lambda nr, nc, B: children(nr, nc, B), lambda nr, nc, B: kbest(nr, nc, B, 2)):
        assert call(0, 5, 1) == E and call(6, 5, 1) == E and call(3, _lib.SH_MAX_N + 1, 1) == E and call(3, 5, -1) == E
        assert call(3, 5, 0) == _lib.SH_OK
    for null in ("C", "pcol", "pv", "p", "forb", "col", "cost", "u", "v"):
        assert children(3, 5, 1, **{null: 1}) == E, null
    for null in ("C", "cols", "costs", "count"):
        assert kbest(3, 5, 1, 2, **{null: 1}) == E, null
    assert kbest(3, 5, 1, 0) == E and kbest(3, 5, 1, 2, work=None) == E
    assert kbest(3, 5, 1, 2, nbytes=int(L.lsap_kbest_work_bytes(3, 5, 1, 2)) - 8) == E
    assert kbest(3, 5, 1, 2, work=ctypes.c_void_p(0x1004)) == E


def test_kbest_front_ends_check_their_arguments_before_the_device(no_gpu):
    C = torch.zeros((2, 3, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="float64 or float32"):
        lsap.kbest_batched(C.long(), 2, free_rows=True)
    with pytest.raises(ValueError, match="k must be"):
        lsap.kbest_batched(C, 0, free_rows=True)
    with pytest.raises(ValueError, match="1024"):
        lsap.kbest_batched(torch.zeros((1, 2, 1025), dtype=torch.float64), 2, free_rows=True)
    col, v = torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.float64)
    p, forb = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(ValueError, match="expected col"):
        lsap.murty_children_batched(C, col, v[:, :3], p, forb, free_rows=True)
    with pytest.raises(TypeError, match="float64"):
        lsap.murty_children_batched(C, col, v.float(), p, forb, free_rows=True)
    with pytest.raises(ValueError, match="wide or square"):
        lsap.murty_children_batched(C.transpose(1, 2), col, v, p, forb, free_rows=True)
    with pytest.raises(ValueError, match="matrix"):
        lsap.kbest_assignments(np.zeros(3), 2, free_rows=True)
    with pytest.raises(ValueError, match="invalid numeric"):
        lsap.kbest_assignments(np.array([[np.nan, 1.0]]), 2, free_rows=True)
    cols, costs = lsap.kbest_assignments(np.zeros((0, 3)), 2, free_rows=True)
    assert cols.shape == (0, 0) and costs.shape == (0,)


def test_kbest_front_ends_of_an_empty_batch(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    cols, costs, count = lsap.kbest_batched(torch.zeros((0, 3, 4), dtype=torch.float32), 3, free_rows=True)
    assert tuple(cols.shape) == (0, 3, 3) and tuple(costs.shape) == (0, 3) and tuple(count.shape) == (0,)
    out = lsap.murty_children_batched(torch.zeros((2, 0, 4), dtype=torch.float64), torch.zeros((2, 0), dtype=torch.int32),
                                      torch.zeros((2, 4), dtype=torch.float64), torch.zeros(2, dtype=torch.int32),
                                      torch.zeros((2, 1), dtype=torch.int64), free_rows=True)
    assert tuple(out[0].shape) == (2, 0, 0) and tuple(out[3].shape) == (2, 0, 4)
