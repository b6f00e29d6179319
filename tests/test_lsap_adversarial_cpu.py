"""The structured and extreme-value LSAP families on the CPU (no GPU calls).

* tests/golden/lsap_adversarial_cases.npz (scipy's answers) against the
  regenerated matrices (sha256) and the CPU oracle, every case;
* the conditions that make the GPU tests of test_lsap_adversarial_gpu.py mean
  something, asserted on the reference alone: the long Dijkstras and the
  nr-hop augmenting path of the Machol-Wien families, the steps outside, inside
  and on the edges of the packed key's window, the int32 extremes.
"""
import functools
import os

import numpy as np
import pytest
import torch

import lsap_families as F
import oracle
from conftest import ROOT, load_npz_cases

SHAPES = [(64, 64), (64, 65), (65, 65), (100, 130), (255, 256), (100, 257), (257, 257), (300, 513), (513, 513),
          (1000, 1024)]
SID = [f"{nr}x{nc}" for nr, nc in SHAPES]
T, L = F.WINDOW_HI, F.WINDOW_LO


@pytest.fixture(scope="module")
def cases():
    return load_npz_cases("lsap_adversarial_cases.npz")


def oracle_matrix(C, dtype):
    return C if dtype == "int64" else F.as_float64(C)


@functools.lru_cache(maxsize=None)
def trace(family, nr, nc):
    return F.sap_trace(F.make(family, "int64", nr, nc))


# --------------------------------------------------------------------------- the fixture
def test_window_constants_are_the_kernels():
    """FB = 10 in sap_solve_mw: LOB = 21, BIAS = 2^42, and the exact argmin
    takes over outside d in [2^32 - 2^42, 2^42 - 2^32)."""
    assert (F.KEY_LOB, F.KEY_BIAS) == (21, 1 << 42)
    assert (L, T) == ((1 << 32) - (1 << 42), (1 << 42) - (1 << 32))
    # the kernel source still says so (a changed window must move the families' edges with it)
    with open(os.path.join(ROOT, "mpi-hungarian-method_amd", "csrc", "santa_hip.hip")) as f:
        src = f.read()
    for line in ("constexpr int LOB = 2 * FB + 1;", "constexpr int64_t BIAS = 1ll << (63 - LOB);",
                 "constexpr uint32_t SAT = SHM << LOB;", "constexpr uint32_t LOW = 1u << LOB;",
                 "const bool exact_step = exact || (uint32_t)(g >> 32) - LOW >= SAT - LOW;",
                 f"sap_solve_mw<NW, K, GlobalLoader<NW, K, S>, {F.KEY_FB}, RECT>"):
        assert line in src, line


def test_fixture_covers_every_family_and_shape(cases):
    _, meta = cases
    have = {(m["family"], m["dtype"], m["nr"], m["nc"]) for m in meta}
    assert have == {(f, d, nr, nc) for f, d in F.all_families() for nr, nc in SHAPES}
    assert len(meta) == len(have) and all(m["seed"] == 0 for m in meta)


@pytest.mark.parametrize("family,dtype", F.all_families(), ids=lambda x: str(x))
def test_fixture_sha_and_oracle(cases, family, dtype):
    z, meta = cases
    seen = 0
    for m in meta:
        if (m["family"], m["dtype"]) != (family, dtype):
            continue
        seen += 1
        nr, nc = m["nr"], m["nc"]
        C = F.make(family, dtype, nr, nc, m["seed"])
        assert F.matrix_sha(C) == m["sha"], m
        want = z[f"col{m['i']}"].astype(np.int64)
        if not m["feasible"]:
            assert (want == -1).all()
            with pytest.raises(ValueError):
                oracle.lsap(oracle_matrix(C, dtype))
            continue
        r, c = oracle.lsap(oracle_matrix(C, dtype))
        assert np.array_equal(r, np.arange(nr)) and np.array_equal(c, want), m
    assert seen == len(SHAPES)


def test_fixture_against_live_scipy(cases):
    """A stale fixture is noticed where scipy is installed."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    z, meta = cases
    picks = [("mw", "int64", 257, 257), ("window_edges", "int64", 100, 130), ("i32_extremes", "int64", 64, 65),
             ("max_overflow", "float64", 65, 65), ("neg_max", "float64", 100, 257), ("multiscale", "float64", 64, 64),
             ("mix_subnormal", "bfloat16", 100, 130), ("dtype_max", "float16", 255, 256)]
    by = {(m["family"], m["dtype"], m["nr"], m["nc"]): m for m in meta}
    for key in picks:
        m = by[key]
        r, c = lsa(F.as_float64(F.make(m["family"], m["dtype"], m["nr"], m["nc"], m["seed"])))
        assert np.array_equal(r, np.arange(m["nr"])) and np.array_equal(c, z[f"col{m['i']}"]), key


# --------------------------------------------------------------------------- generators
def test_generators_are_pure_and_typed():
    for family, dtype in F.all_families():
        a, b, c = (F.make(family, dtype, 64, 65, s) for s in (0, 0, 1))
        assert F.matrix_sha(a) == F.matrix_sha(b), family
        if family not in F.SEEDLESS:
            assert F.matrix_sha(a) != F.matrix_sha(c), family
        if dtype in F.NARROW:
            assert isinstance(a, torch.Tensor) and a.dtype == F.NARROW[dtype] and tuple(a.shape) == (64, 65)
        else:
            assert a.dtype == np.dtype(dtype) and a.shape == (64, 65)


def test_instances_differ_and_start_at_the_fixture():
    for family, dtype in (("mw", "int64"), ("two_scale43", "int64"), ("mw_sqrt", "bfloat16")):
        shas = [F.matrix_sha(F.instance(family, dtype, 64, 65, k)) for k in range(3)]
        assert len(set(shas)) == 3 and shas[0] == F.matrix_sha(F.make(family, dtype, 64, 65, 0))


def test_integer_family_ranges():
    for family in F.INT_FAMILIES:
        for nr, nc in ((64, 65), (1000, 1024)):
            C = F.make(family, "int64", nr, nc)
            assert max(int(C.max()), -int(C.min())) < 1 << 50, family
            if family in F.INT32_FAMILIES:
                assert F.I32_MIN <= int(C.min()) and int(C.max()) <= F.I32_MAX, family
    for nr, nc in SHAPES:
        C = F.make("i32_extremes", "int64", nr, nc)
        assert int(C.min()) == F.I32_MIN and int(C.max()) == F.I32_MAX
        for s in F.I32_SPECIALS:
            assert (C == s).any(), s
        assert (F.make("mw_neg", "int64", nr, nc) < 0).all()


def test_float_family_extremes():
    tiny = np.finfo(np.float64).tiny
    for nr, nc in ((64, 65), (130, 130)):
        C = F.make("max_overflow", "float64", nr, nc)
        assert np.isfinite(C).all() and (C == F.DBL_MAX).mean() > 0.2
        with np.errstate(over="ignore"):
            assert np.isinf(C[0] + C[1]).any()  # (the sums scipy forms overflow)
        C = F.make("neg_max", "float64", nr, nc)
        assert np.isfinite(C).all() and (C == -F.DBL_MAX).mean() > 0.2
        C = F.make("subnormal64", "float64", nr, nc)
        assert C.max() == 8 * 5e-324 and ((C > 0) & (C < tiny)).mean() > 0.5
        C = np.abs(F.make("multiscale", "float64", nr, nc))
        assert np.log10(C.max()) - np.log10(C[C > 0].min()) > 590
        assert F.make("huge", "float64", nr, nc).max() > 0.99e308


@pytest.mark.parametrize("dtype", sorted(F.NARROW))
def test_narrow_family_extremes(dtype):
    dt = F.NARROW[dtype]
    fi = torch.finfo(dt)
    for nr, nc in ((64, 65), (130, 130)):
        t = F.make("subnormal", dtype, nr, nc)
        assert float(t.double().max()) == 7 * F.smallest_subnormal(dt) and int(F._is_subnormal(t).sum()) > nr * nc // 2
        t = F.make("mix_subnormal", dtype, nr, nc)
        assert int(F._is_subnormal(t).sum()) > nr * nc // 4 and bool((t < 0).any())
        assert float(t.double().abs().max()) > fi.smallest_normal  # (normals next to the subnormals)
        t = F.make("dtype_max", dtype, nr, nc)
        assert bool(torch.isfinite(t).all()) and bool((t == fi.max).any()) and bool((t == -fi.max).any())
    t = F.make("mix_subnormal", dtype, 130, 130)
    assert int(F._is_subnormal(t).sum()) > 4000
    # bfloat16 has 128 values per binade: the 257^2 entries in [1, 257] share at
    # most 8 * 128 + 1 values, so the long-path family is full of ties
    if dtype == "bfloat16":
        assert np.unique(F.make("mw_sqrt", dtype, 257, 257).double().numpy()).size <= 8 * 128 + 1


# --------------------------------------------------------------------------- what the GPU tests rely on
@pytest.mark.parametrize("family,dtype", [("mw", "int64"), ("mw_neg", "int64"), ("mw_tenths", "float64"),
                                          ("mw_sqrt", "float64")])
def test_long_dijkstras(family, dtype):
    """About nr / 2 Dijkstra steps per row (noise: 7 to 22)."""
    for nr, nc in SHAPES:
        st = np.zeros(2, dtype=np.uint64)
        oracle.lsap(oracle_matrix(F.make(family, dtype, nr, nc), dtype), st)
        assert int(st[0]) / nr >= 0.45 * nr, (family, nr, nc, int(st[0]))


@pytest.mark.parametrize("n", [64, 65, 257, 513])
def test_mw_longest_path_is_nr_hops(n):
    """The bound of sap_solve_mw_f64's augmenting walk, reached exactly."""
    col, d, first, longest = trace("mw", n, n)
    assert longest == n
    assert np.array_equal(col, oracle.lsap(F.make("mw", "int64", n, n))[1])
    assert int(first.sum()) == n and d.size >= 0.45 * n * n


@pytest.mark.parametrize("nr,nc", [(100, 128), (64, 129)])
def test_window_conditions_of_the_large_batch_matrices(nr, nc):
    """The matrices the one-wave large-batch GPU test repeats over its batch
    (six seeds per family) leave the window on both sides and hit its edges."""
    above = below = 0
    edges = set()
    for seed in range(6):
        d = F.sap_trace(F.make("two_scale43", "int64", nr, nc, seed))[1]
        above += int((d >= T).sum())
        d = F.sap_trace(F.make("neg_cols", "int64", nr, nc, seed))[1]
        below += int((d < L).sum())
        _, d, first, _ = F.sap_trace(F.make("window_edges", "int64", nr, nc, seed))
        edges |= set(d[first].tolist())
    assert above >= 5 and below >= 5 and set(F.EDGE_OFFSETS[:6]) <= edges, (above, below)


@pytest.mark.parametrize("nr,nc", SHAPES, ids=SID)
def test_tracer_equals_oracle_and_window_conditions(nr, nc):
    for family in ("two_scale42", "two_scale43", "two_scale45", "neg_cols", "window_edges", "i32_extremes"):
        col, d, first, _ = trace(family, nr, nc)
        st = np.zeros(2, dtype=np.uint64)
        _, oc = oracle.lsap(F.make(family, "int64", nr, nc), st)
        assert np.array_equal(col, oc), family
        assert d.size == int(st[0]), family
    # packed and exact steps inside one solve: a few above the window, most in it
    _, d, _, _ = trace("two_scale43", nr, nc)
    assert int((d >= T).sum()) >= 5 and int(((d >= L) & (d < T)).sum()) >= 0.75 * d.size, (d >= T).sum()
    # the low band: steps far below minVal
    _, d, _, _ = trace("neg_cols", nr, nc)
    assert int((d < L).sum()) >= 5, (d < L).sum()
    # winners on, and next to, either edge of the window
    _, d, first, _ = trace("window_edges", nr, nc)
    assert set(F.EDGE_OFFSETS[:6]) <= set(d[first].tolist())
