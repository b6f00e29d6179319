"""CPU side of the batched LSAP above 1024 columns (solve_batched_large,
check_duals_large, linear_sum_assignment_large and the lsap_*_large_ entries):
the fixtures, the host checks of the twelve C-ABI entries (made before any
device call, so they run here), the int64 bound, and the Python front end with
the solver stubbed by the oracle."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_duals_ref as R  # noqa: E402
import lsap_families as F  # noqa: E402
import lsap_large_families as L  # noqa: E402
import oracle  # noqa: E402
from conftest import GOLDEN, load_npz_cases  # noqa: E402
from santa_hip import _lib, lsap  # noqa: E402

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
FLOAT_SUFFIXES = SUFFIXES[2:]
FIXTURE_CASES = L.fixture_cases()


@pytest.fixture(autouse=True)
def large_surface():
    """Everything here is about the large surface: without it nothing passes."""
    assert hasattr(lsap, "solve_batched_large") and hasattr(_lib, "SH_MAX_N_LARGE"), \
        "santa_hip has no solve_batched_large / SH_MAX_N_LARGE"


@functools.lru_cache(maxsize=None)
def large_cases():
    return load_npz_cases("lsap_large_cases.npz")


# --------------------------------------------------------------------------- fixtures
def test_fixture_lists_every_case_in_order():
    z, meta = large_cases()
    assert [(m["family"], m["dtype"], m["nr"], m["nc"]) for m in meta] == FIXTURE_CASES
    assert [m["feasible"] for m in meta] == [f != "inf_row" for f, _, _, _ in FIXTURE_CASES]


@pytest.mark.parametrize("i", range(len(FIXTURE_CASES)), ids=["-".join(str(x) for x in c) for c in FIXTURE_CASES])
def test_generators_reproduce_their_hash_and_the_oracle_agrees_with_scipy(i):
    z, meta = large_cases()
    m = meta[i]
    C = L.instance(m["family"], m["dtype"], m["nr"], m["nc"], 0)
    assert C.shape == (m["nr"], m["nc"]) and str(C.dtype) == m["dtype"]
    assert F.matrix_sha(C) == m["sha"], "the generator changed: rewrite the fixture"
    want = z[f"col{i}"].astype(np.int64)
    if not m["feasible"]:
        assert (want == -1).all()
        with pytest.raises(ValueError, match="infeasible"):
            oracle.lsap(C)
        return
    r, c = oracle.lsap(C)
    assert np.array_equal(r, np.arange(m["nr"])) and np.array_equal(c, want)


def test_recorded_replays_belong_to_the_generators():
    z = np.load(os.path.join(GOLDEN, "lsap_large_replay.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    assert [tuple(m["key"]) for m in meta] == L.recorded_replays()
    for i, m in enumerate(meta):
        family, dtype, nr, nc, k = m["key"]
        assert z[f"col{i}"].shape == (nr,) and z[f"u{i}"].shape == (nr,) and z[f"v{i}"].shape == (nc,)
        assert str(z[f"u{i}"].dtype) == dtype and str(z[f"v{i}"].dtype) == dtype
    # one of them replayed again (the shortest), and every instance 0 against scipy's fixture
    i = [tuple(m["key"]) for m in meta].index(("mw", "int64", 300, 2048, 1))
    C = L.instance("mw", "int64", 300, 2048, 1)
    assert F.matrix_sha(C) == meta[i]["sha"]
    col, u, v = R.replay(C)
    assert np.array_equal(col, z[f"col{i}"]) and np.array_equal(u, z[f"u{i}"]) and np.array_equal(v, z[f"v{i}"])
    zc, mc = large_cases()
    by_case = {(m["family"], m["dtype"], m["nr"], m["nc"]): zc[f"col{m['i']}"] for m in mc}
    for i, m in enumerate(meta):
        family, dtype, nr, nc, k = m["key"]
        if k == 0:
            assert np.array_equal(z[f"col{i}"], by_case[family, dtype, nr, nc]), m["key"]


def test_window_constants_of_the_12_bit_key():
    assert L.WINDOW_HI12 == (1 << 38) - (1 << 32) and L.WINDOW_LO12 == (1 << 32) - (1 << 38)
    C = L.window_edges12(14, 2049)
    assert C.min(axis=1).tolist() == [L.EDGE_OFFSETS12[i % 7] for i in range(14)]
    assert int(np.abs(C).max()) < (1 << 48)
    for big in (38, 39, 41):
        C = L.INT_FAMILIES[f"two_scale{big}"](20, 2049)
        assert (1 << big) <= int(C.max()) < (1 << big) + (1 << 16) and int(C.min()) >= 0
    T = L.tiny_range(50, 2049)
    assert T.min() == 0 and T.max() == 3
    for f in L.INT32_FAMILIES:
        for nr, nc in ((300, 4096), (1025, 1025)):
            C = L.INT_FAMILIES[f](nr, nc)
            assert C.min() >= F.I32_MIN and C.max() <= F.I32_MAX
    for name, dt in F.NARROW.items():  # the cross-dtype families are exact in every narrow dtype
        for fam in ("tiny_range", "inf_band", "inf_row"):
            C = L.F64_FAMILIES[fam](40, 1100)
            assert np.array_equal(L.narrow(C, dt).double().numpy(), C), (fam, name)
    assert np.isinf(L.inf_row(300, 2049)).all(axis=1).sum() == 1


# --------------------------------------------------------------------------- C-ABI host checks
def _ptr(x=4096):
    """A non-null pointer the entry never dereferences: every call here is
    turned down by a host check (or has B == 0)."""
    return ctypes.c_void_p(x)


def _solve(suf, nr, nc, B, C=True, col=True, cost=True, u=True, v=True, flags=0):
    f = getattr(_lib.lib(), "lsap_solve_large_" + suf)
    p = lambda on: _ptr() if on else None  # noqa: E731
    return f(p(C), nr, nc, B, None, p(col), p(cost), p(u), p(v), flags, None)


def _check(suf, nr, nc, B, C=True, col=True, u=True, v=True, slack=True, flg=True):
    f = getattr(_lib.lib(), "lsap_check_duals_large_" + suf)
    p = lambda on: _ptr() if on else None  # noqa: E731
    return f(p(C), nr, nc, B, None, p(col), p(u), p(v), p(slack), p(flg), None)


def test_library_exports_the_twelve_entries():
    assert _lib.SH_MAX_N_LARGE == 4096 and _lib.SH_MAX_N == 1024
    for suf in SUFFIXES:
        assert _lib.SIGNATURES["lsap_solve_large_" + suf] == _lib.SIGNATURES["lsap_solve_batched_duals_" + suf]
        assert _lib.SIGNATURES["lsap_check_duals_large_" + suf] == _lib.SIGNATURES["lsap_check_duals_" + suf]
        assert hasattr(_lib.lib(), "lsap_solve_large_" + suf) and hasattr(_lib.lib(), "lsap_check_duals_large_" + suf)


@pytest.mark.parametrize("suf", SUFFIXES)
def test_large_entries_check_their_arguments_on_the_host(suf):
    E = _lib.SH_ERR_ARGS
    for call in (_solve, _check):
        assert call(suf, 10, 4097, 1) == E and "4096" in _lib.last_error()
        assert call(suf, 0, 10, 1) == E
        assert call(suf, -1, 10, 1) == E
        assert call(suf, 11, 10, 1) == E and "nr > nc" in _lib.last_error()
        assert call(suf, 4097, 4097, 1) == E
        assert call(suf, 10, 2000, -1) == E and "B < 0" in _lib.last_error()
        assert call(suf, 10, 2000, 1, C=False) == E
        assert call(suf, 10, 2000, 1, col=False) == E
        # (the checks come first for B == 0 too; then nothing is needed)
        assert call(suf, 10, 4097, 0) == E and call(suf, 11, 10, 0) == E
    assert _solve(suf, 10, 2000, 1, u=False) == E and "both or neither" in _lib.last_error()
    assert _solve(suf, 10, 2000, 1, v=False) == E
    assert _solve(suf, 10, 100, 1, u=False) == E  # (below the old limit too)
    for miss in ("u", "v", "slack", "flg"):
        assert _check(suf, 10, 2000, 1, **{miss: False}) == E, miss
    assert _solve(suf, 4096, 4096, 0) == _lib.SH_OK
    assert _solve(suf, 4096, 4096, 0, C=False, col=False, cost=False, u=False, v=False) == _lib.SH_OK
    assert _solve(suf, 1, 4096, 0, u=False, v=False) == _lib.SH_OK
    assert _check(suf, 4096, 4096, 0) == _lib.SH_OK
    assert _check(suf, 4096, 4096, 0, C=False, col=False, u=False, v=False, slack=False, flg=False) == _lib.SH_OK


@pytest.mark.parametrize("suf", FLOAT_SUFFIXES)
def test_large_float_entries_check_the_kernel_flags(suf):
    E, MW, SW = _lib.SH_ERR_ARGS, _lib.SH_FLAG_F64_MW, _lib.SH_FLAG_F64_SW
    for nc in (100, 1024, 1025, 4096):
        assert _solve(suf, 10, nc, 1, flags=MW | SW) == E and "exclude" in _lib.last_error()
        assert _solve(suf, 10, nc, 0, flags=MW | SW) == E
    assert _solve(suf, 10, 1025, 1, flags=SW) == E and "one-wave" in _lib.last_error()
    assert _solve(suf, 10, 4096, 0, flags=SW) == E
    assert _solve(suf, 10, 1024, 0, flags=SW) == _lib.SH_OK
    assert _solve(suf, 10, 4096, 0, flags=MW) == _lib.SH_OK


def test_existing_entries_keep_their_limit():
    L_ = _lib.lib()
    p = _ptr()
    assert L_.lsap_solve_batched_rect_i64(p, 10, 1025, 1, None, p, p, 0, None) == _lib.SH_ERR_ARGS
    assert "[1, 1024]" in _lib.last_error()
    assert L_.lsap_solve_batched_duals_f64(p, 10, 1025, 1, None, p, p, p, p, 0, None) == _lib.SH_ERR_ARGS
    assert "[1, 1024]" in _lib.last_error()
    assert L_.lsap_check_duals_i32(p, 10, 1025, 1, None, p, p, p, p, p, None) == _lib.SH_ERR_ARGS
    assert "[1, 1024]" in _lib.last_error()
    assert L_.lsap_solve_batched_f64(p, 1025, 1, p, p, 0, None) == _lib.SH_ERR_ARGS


# --------------------------------------------------------------------------- the int64 bound
def test_int64_cost_limit():
    assert [lsap.int64_cost_limit(n) for n in (1, 1024, 1025, 2000, 4096)] == \
        [1 << 50, 1 << 50, 1 << 48, 1 << 48, 1 << 48]
    # the argument of the bound: a factor 4n below 2^62
    assert 4 * 1024 * (1 << 50) == 1 << 62 and 4 * 4096 * (1 << 48) == 1 << 62
    assert lsap.INT64_COST_LIMIT == 1 << 50


def test_int64_range_check_names_the_bound(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    big = torch.zeros((1, 2, 1025), dtype=torch.int64)
    big[0, 1, 7] = -(1 << 48)
    with pytest.raises(ValueError, match=r"2\*\*48"):
        lsap.solve_batched_large(big)
    with pytest.raises(ValueError, match=r"2\*\*48"):
        lsap.solve_batched_large(big.transpose(1, 2), duals=True)
    small = torch.zeros((1, 2, 1024), dtype=torch.int64)
    small[0, 0, 0] = 1 << 50
    with pytest.raises(ValueError, match=r"2\*\*50"):
        lsap.solve_batched_large(small)


# --------------------------------------------------------------------------- the front end without a GPU
def test_large_front_end_shape_surface_without_gpu(monkeypatch):
    """linear_sum_assignment_large's host side with the solver stubbed by the
    oracle (as test_lsap_rect_cpu does for linear_sum_assignment): what it
    hands down, the ordering it returns, the empty and the over-size cases."""
    seen = []

    def fake(C, with_cost=True, flags=0, duals=False):
        seen.append((tuple(C.shape), C.dtype))
        B, nr, nc = C.shape
        assert nr <= nc
        _, col = oracle.lsap(C[0].numpy())
        out = (torch.from_numpy(col.astype(np.int32)).unsqueeze(0), None)
        if duals:
            _, u, v = R.replay(C[0].numpy())
            out += (torch.from_numpy(u).unsqueeze(0), torch.from_numpy(v).unsqueeze(0))
        return out

    monkeypatch.setattr(lsap, "solve_batched_large", fake)
    rng = np.random.default_rng(3)
    for shape in ((2, 1025), (1025, 2), (3, 4096), (4096, 3), (5, 5)):
        for C in (rng.integers(0, 100, size=shape), rng.random(shape)):
            for maximize in (False, True):
                r, c = lsap.linear_sum_assignment_large(C, maximize=maximize, device="cpu")
                assert seen[-1] == ((1, min(shape), max(shape)), torch.int64 if C.dtype == np.int64 else torch.float64)
                wr, wc = oracle.lsap(-C if maximize else C)
                assert r.dtype == np.int64 and c.dtype == np.int64
                assert np.array_equal(r, wr) and np.array_equal(c, wc), (shape, maximize)
                r2, c2, u, v = lsap.linear_sum_assignment_large(C, maximize=maximize, device="cpu", duals=True)
                assert np.array_equal(r2, r) and np.array_equal(c2, c)
                assert u.shape == (shape[0],) and v.shape == (shape[1],)
                S = C - u[:, None] - v[None, :]
                if C.dtype == np.int64:
                    assert ((S <= 0) if maximize else (S >= 0)).all() and not S[r, c].any()
    n = len(seen)
    for shape in ((2, 4097), (4097, 2)):
        with pytest.raises(ValueError, match="4096"):
            lsap.linear_sum_assignment_large(np.zeros(shape), device="cpu")
    for shape in ((0, 0), (0, 5), (5, 0)):
        r, c = lsap.linear_sum_assignment_large(np.zeros(shape), device="cpu")
        assert r.dtype == np.int64 and c.dtype == np.int64 and r.size == 0 and c.size == 0
        z = lsap.linear_sum_assignment_large(np.zeros(shape), device="cpu", duals=True)
        assert [a.size for a in z] == [0, 0, shape[0], shape[1]]
    assert len(seen) == n  # none of these reached the solver
    with pytest.raises(ValueError, match="invalid numeric"):
        lsap.linear_sum_assignment_large(np.full((2, 1025), np.nan), device="cpu")
    with pytest.raises(ValueError, match="invalid numeric"):
        lsap.linear_sum_assignment_large(np.full((2, 1025), -np.inf), device="cpu")
    # an integer matrix too wide for the exact route goes down as float64
    lsap.linear_sum_assignment_large(np.full((2, 1025), 1 << 45, dtype=np.int64), device="cpu")
    assert seen[-1] == ((1, 2, 1025), torch.float64)


def test_batched_front_ends_check_sizes_before_the_device(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    for shape in ((1, 2, 4097), (1, 4097, 2)):
        C = torch.zeros(shape, dtype=torch.int32)
        with pytest.raises(ValueError, match="4096"):
            lsap.solve_batched_large(C)
        with pytest.raises(ValueError, match="4096"):
            lsap.check_duals_large(C, torch.zeros(shape[:2], dtype=torch.int32),
                                   torch.zeros(shape[:2], dtype=torch.int64),
                                   torch.zeros((1, shape[2]), dtype=torch.int64))
    # empty batches and empty matrices need no device either
    for shape in ((0, 5, 2000), (2, 0, 2000), (2, 2000, 0)):
        C = torch.zeros(shape, dtype=torch.float32)
        col, cost, u, v = lsap.solve_batched_large(C, duals=True)
        assert tuple(col.shape) == shape[:2] and bool((col == -1).all()) and not cost.any()
        assert tuple(u.shape) == shape[:2] and tuple(v.shape) == (shape[0], shape[2])
        assert cost.dtype == u.dtype == v.dtype == torch.float64
        out = lsap.check_duals_large(C, col, u, v)
        assert [tuple(t.shape) for t in out] == [(shape[0],)] * 4
    with pytest.raises(ValueError, match="padded wide"):
        lsap.solve_batched_large(torch.zeros((1, 2000, 5)), shapes=[(1, 1)])
    with pytest.raises(ValueError, match="outside the padded"):
        lsap.solve_batched_large(torch.zeros((1, 5, 2000)), shapes=[(1, 2001)])
    with pytest.raises(TypeError):
        lsap.solve_batched_large(torch.zeros((1, 5, 2000), dtype=torch.int16))


def test_the_old_functions_still_stop_at_1024(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    for shape in ((2, 1025), (1025, 2)):
        with pytest.raises(ValueError, match="1024"):
            lsap.linear_sum_assignment(np.zeros(shape), device="cpu")
        with pytest.raises(ValueError, match="1024"):
            lsap.linear_sum_assignment_duals(np.zeros(shape), device="cpu")
        C = torch.zeros((1,) + shape, dtype=torch.int64)
        with pytest.raises(ValueError, match="> 1024"):
            lsap.solve_batched(C)
        with pytest.raises(ValueError, match="> 1024"):
            lsap.check_duals(C, torch.zeros((1, shape[0]), dtype=torch.int32),
                             torch.zeros((1, shape[0]), dtype=torch.int64),
                             torch.zeros((1, shape[1]), dtype=torch.int64))


def test_package_exports_the_large_surface():
    import santa_hip
    for name in ("solve_batched_large", "check_duals_large", "linear_sum_assignment_large"):
        assert getattr(santa_hip, name) is getattr(lsap, name) and name in santa_hip.__all__


# --------------------------------------------------------------------------- resources
def test_large_kernels_exist_and_use_no_scratch(tmp_path):
    """The code object holds the 12-bit-key instantiations of the two solvers
    and the 4096-column certificate, none of them with private memory."""
    from test_kernel_resources_cpu import _kernel_meta
    meta = _kernel_meta(tmp_path)
    large = {k: v for k, v in meta.items()
             if (("lsap_f64_mw_kernel" in k or "lsap_i64_kernel" in k) and "Li12E" in k) or
             (("lsap_cert_kernel" in k or "lsap_slack_kernel" in k) and "Li4096E" in k)}
    # 3 configurations x 2 stored types x with / without duals; 3 x 4 x 2; 6 + 12 certificate kernels
    assert sum("lsap_i64_kernel" in k for k in large) == 12
    assert sum("lsap_f64_mw_kernel" in k for k in large) == 24
    assert sum("lsap_cert_kernel" in k for k in large) == 6 and sum("lsap_slack_kernel" in k for k in large) == 12
    assert not {k: v for k, v in large.items() if v}, "kernels with private (scratch) memory"
    assert not {k: v for k, v in meta.items() if "lsap_" in k and v}
