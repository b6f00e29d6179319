"""Batched bottleneck assignment on the GPU against the host references of
lbap_ref.py: col bit for bit the reference loop's, value equal to the loop's
and to the independent threshold search's, in every forced kernel design and
in the default one."""
import functools

import numpy as np
import pytest
import torch

import lsap_families
from lbap_ref import lbap_ref, threshold_value
from santa_hip import _lib, linear_bottleneck_assignment, solve_bottleneck_batched

pytestmark = pytest.mark.gpu

I64, I32 = np.iinfo(np.int64), np.iinfo(np.int32)
TORCH = {"i64": torch.int64, "i32": torch.int32, "f64": torch.float64, "f32": torch.float32,
         "f16": torch.float16, "bf16": torch.bfloat16}
NUMPY = {"i64": np.int64, "i32": np.int32, "f64": np.float64, "f32": np.float32, "f16": np.float16}
BITS = {8: torch.int64, 4: torch.int32, 2: torch.int16}


def designs(nc):
    """(name, flags) of the launch table's designs at nc columns: the default,
    and each forced one that exists there."""
    out = [("default", 0), ("mw", _lib.SH_FLAG_LBAP_MW)]
    if nc <= _lib.SH_MAX_N:
        out.append(("sw", _lib.SH_FLAG_LBAP_SW))
    return out


def to_host(t):
    """A tensor as numpy; bfloat16 widened to float32 (exact, same order)."""
    t = t.cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


def bits(t):
    return t.cpu().contiguous().view(BITS[t.element_size()])


def solve(C, flags=0, **kw):
    col, value = solve_bottleneck_batched(C.cuda(), flags=flags, **kw)
    torch.cuda.synchronize()
    return col.cpu().numpy(), value.cpu()


def check_against_refs(C, refs, maximize=False, shapes=None):
    """C: torch [B, NR, NC] (host); refs: per instance (col [NR], value) of the
    reference.  Every design returns exactly that."""
    for name, flags in designs(C.shape[2]):
        col, value = solve(C, flags, maximize=maximize, shapes=shapes)
        v = to_host(value)
        for b, (rcol, rval) in enumerate(refs):
            assert np.array_equal(col[b], rcol), (name, b, np.flatnonzero(col[b] != rcol)[:8])
            assert v[b] == rval, (name, b, v[b], rval)


def perm_batch(base, B, seed):
    """B row permutations of one matrix (the first is the matrix itself)."""
    rng = np.random.default_rng(seed)
    return np.stack([base if b == 0 else base[rng.permutation(base.shape[0])] for b in range(B)])


def refs_of(Cb, maximize=False, threshold=True):
    out = []
    for C in Cb:
        col, value, _, _ = lbap_ref(C, maximize)
        if threshold and C.shape[0]:
            want = threshold_value(C, maximize)
            assert value == want, (value, want)
        out.append((col, value))
    return out


# --------------------------------------------------------------------------- shapes and families
SHAPES = [(1, 1), (1, 5), (2, 2), (3, 7), (63, 64), (64, 64), (64, 65), (65, 65), (255, 256), (256, 256),
          (257, 257), (1023, 1024), (1024, 1024), (1025, 1025),
          # at and past every seam of the launch table that is not above: the one-wave
          # design's 128 and 512 columns, the multi-wave design's 512 and 2048
          (128, 128), (129, 129), (512, 512), (513, 513), (2048, 2048), (2049, 2049)]
SMALL = [(3, 7), (63, 64), (65, 65), (255, 256), (257, 257)]


@pytest.mark.parametrize("nr,nc", SHAPES)
def test_uniform_random(nr, nc):
    rng = np.random.default_rng([1, nr, nc])
    base = rng.integers(-(1 << 30), 1 << 30, size=(nr, nc))  # exact in int32 and in float64
    Cb = perm_batch(base, 4 if nc <= 257 else 2, [2, nr, nc])
    if nc <= 1025:
        refs = refs_of(Cb)
        for dt in ("i32", "f64"):
            check_against_refs(torch.from_numpy(Cb.astype(NUMPY[dt])), refs)
        return
    # beyond: the reference loop takes ten seconds an instance, so the result's
    # own properties and the threshold search (one design exists here)
    want = [threshold_value(C) for C in Cb]
    for dt in ("i32", "f64"):
        for name, flags in designs(nc):
            col, value = solve(torch.from_numpy(Cb.astype(NUMPY[dt])), flags)
            for b in range(len(Cb)):
                assert np.unique(col[b]).size == nr
                assert col[b].min() >= 0 and col[b].max() < nc
                assert Cb[b, np.arange(nr), col[b]].max() == value.numpy()[b] == want[b], (name, dt, b)


@pytest.mark.parametrize("nr,nc", SMALL + [(1024, 1024)])
def test_ties(nr, nc):
    rng = np.random.default_rng([3, nr, nc])
    base = rng.integers(0, 4, size=(nr, nc))
    for dt in ("i64", "f32"):
        Cb = perm_batch(base.astype(NUMPY[dt]), 2 if nc > 257 else 4, [4, nr, nc])
        check_against_refs(torch.from_numpy(Cb), refs_of(Cb))


@pytest.mark.parametrize("nr,nc", SMALL + [(1024, 1024), (1025, 1025)])
def test_all_equal(nr, nc):
    for dt, x in (("i32", -7), ("f16", 2.5)):
        Cb = np.full((2, nr, nc), x, dtype=NUMPY[dt])
        check_against_refs(torch.from_numpy(Cb), refs_of(Cb))


@pytest.mark.parametrize("nr,nc", [(64, 64), (65, 65), (200, 257)])
def test_machol_wien_long_paths(nr, nc):
    """(i + 1) (j + 1): searches of at least nr / 2 steps and augmenting paths
    of at least nr / 2 hops (49 and 41 at 64 x 64), from the reference's own
    counters."""
    base = lsap_families.mw(nr, nc)
    _, _, steps, hops = lbap_ref(base)
    assert steps >= nr / 2 and hops >= nr / 2, (steps, hops)
    for dt in ("i64", "f32"):
        Cb = perm_batch(base.astype(NUMPY[dt]), 3, [5, nr, nc])
        check_against_refs(torch.from_numpy(Cb), refs_of(Cb))


def inf_pattern(nr, nc, seed, dtype):
    """About half +inf around a finite random permutation: feasible."""
    rng = np.random.default_rng([6, nr, nc, seed])
    C = rng.integers(0, 1000, size=(nr, nc)).astype(dtype)
    keep = rng.random((nr, nc)) < 0.5
    keep[np.arange(nr), rng.permutation(nc)[:nr]] = True
    C[~keep] = np.inf
    return C


@pytest.mark.parametrize("nr,nc", SMALL)
def test_inf_patterns_feasible(nr, nc):
    for dt in ("f64", "f32", "f16"):
        Cb = perm_batch(inf_pattern(nr, nc, 0, NUMPY[dt]), 3, [7, nr, nc])
        refs = refs_of(Cb)
        assert all(np.isfinite(v) and (c >= 0).all() for c, v in refs)
        check_against_refs(torch.from_numpy(Cb), refs)


@pytest.mark.parametrize("nr,nc", [(2, 2), (3, 7), (65, 65), (255, 256), (257, 300)])
def test_inf_patterns_infeasible(nr, nc):
    rng = np.random.default_rng([8, nr, nc])
    for dt in ("f64", "f32", "bf16"):
        base = rng.integers(0, 100, size=(nr, nc)).astype(np.float32)
        row_inf = base.copy()
        row_inf[nr // 2] = np.inf                      # a row of all +inf
        clash = base.copy()                            # two rows whose only finite entry is the same column
        clash[[0, nr - 1]] = np.inf
        clash[[0, nr - 1], nc // 3] = 5.0
        fine = base.copy()
        fine[nr // 2, : nc - 1] = np.inf               # (and a feasible neighbour in the same launch)
        Cb = np.stack([row_inf, clash, fine])
        refs = refs_of(Cb)
        assert [bool((c < 0).all()) for c, _ in refs] == [True, True, False]
        assert refs[0][1] == np.inf and refs[1][1] == np.inf
        check_against_refs(torch.from_numpy(Cb).to(TORCH[dt]), refs)


# --------------------------------------------------------------------------- dtypes
@pytest.mark.parametrize("nr,nc", [(5, 9), (64, 65), (130, 257)])
def test_six_dtypes_agree_and_value_is_an_element(nr, nc):
    rng = np.random.default_rng([9, nr, nc])
    Cb = perm_batch(rng.integers(-100, 101, size=(nr, nc)), 3, [10, nr, nc])  # exact in every dtype
    refs = refs_of(Cb.astype(np.int64))
    for dt, tdt in TORCH.items():
        C = torch.from_numpy(Cb).to(tdt)
        check_against_refs(C, refs)
        col, value = solve(C)
        chosen = torch.gather(C, 2, torch.from_numpy(col).long().unsqueeze(2)).squeeze(2)
        assert value.dtype == tdt
        assert (bits(chosen) == bits(value).unsqueeze(1)).any(1).all(), dt


def from_bits(x, tdt):
    return torch.tensor(x, dtype=BITS[torch.empty(0, dtype=tdt).element_size()]).view(tdt)


EXTREMES = [  # (dtype, the extreme's bits, whether it is the dtype's top (a whole row of it) or bottom (a permutation))
    ("i64", I64.max, True), ("i64", I64.min, False), ("i32", I32.max, True), ("i32", I32.min, False),
    ("f64", np.array(np.finfo(np.float64).max).view(np.int64).item(), True),
    ("f32", np.array(np.finfo(np.float32).max).view(np.int32).item(), True),
    ("f16", 0x7BFF, True), ("bf16", 0x7F7F, True),
    ("f64", np.array(-np.inf).view(np.int64).item(), False), ("f32", np.array(-np.inf, np.float32).view(np.int32).item(), False),
    ("f16", 0xFC00 - (1 << 16), False), ("bf16", 0xFF80 - (1 << 16), False),
    ("f64", 1, None), ("f32", 1, None), ("f16", 1, None), ("bf16", 1, None),  # the least subnormal, over zeros and negatives
]


@pytest.mark.parametrize("dt,xbits,top", EXTREMES)
def test_extremes_as_the_bottleneck(dt, xbits, top):
    tdt = TORCH[dt]
    x = from_bits([xbits], tdt)[0]
    nr, nc = 6, 9
    rng = np.random.default_rng([11, abs(xbits) % 1000003])
    Cs = []
    for b in range(3):
        if top is False:  # x on a permutation, everything else larger: the optimum takes the permutation
            C = torch.from_numpy(rng.integers(-50, 50, size=(nr, nc))).to(tdt)
            C[torch.arange(nr), torch.from_numpy(rng.permutation(nc)[:nr])] = x
        else:  # one row is x throughout, everything else smaller
            lo, hi = (-50, 50) if top else (-3, 1)
            C = torch.from_numpy(rng.integers(lo, hi, size=(nr, nc))).to(tdt)
            C[int(rng.integers(nr))] = x
        Cs.append(C)
    C = torch.stack(Cs)
    refs = refs_of(to_host(C))
    check_against_refs(C, refs)
    _, value = solve(C)
    assert (bits(value) == xbits).all(), (dt, bits(value), xbits)


def test_int64_of_magnitude_2_62():
    """The min-sum solver refuses |C| >= 2^50; comparisons have no such limit."""
    rng = np.random.default_rng(12)
    Cb = rng.integers(-(1 << 62), 1 << 62, size=(3, 70, 90)) | (1 << 61)
    Cb[1] = rng.integers(I64.min, I64.max, size=(70, 90), endpoint=True)
    check_against_refs(torch.from_numpy(Cb), refs_of(Cb))


# --------------------------------------------------------------------------- maximize
@pytest.mark.parametrize("nr,nc", [(4, 6), (65, 70), (200, 257)])
def test_maximize_is_the_reversed_order(nr, nc):
    rng = np.random.default_rng([13, nr, nc])
    Ci = rng.integers(-5, 6, size=(3, nr, nc)).astype(np.int64)
    Ci[rng.random(Ci.shape) < 0.2] = I64.min
    Ci[rng.random(Ci.shape) < 0.2] = I64.max
    Ci[0, nr // 2] = I64.min               # a whole row of it: the value of instance 0
    refs = [(c, ~v) for c, v in refs_of(~Ci)]
    assert refs[0][1] == I64.min
    check_against_refs(torch.from_numpy(Ci), refs, maximize=True)
    Ci32 = rng.integers(I32.min, I32.max, size=(3, nr, nc), endpoint=True).astype(np.int32)
    check_against_refs(torch.from_numpy(Ci32), [(c, ~v) for c, v in refs_of(~Ci32)], maximize=True)
    # floats: -inf is forbidden, +inf the best possible cost
    Cf = rng.integers(0, 50, size=(3, nr, nc)).astype(np.float32)
    Cf[rng.random(Cf.shape) < 0.3] = -np.inf
    Cf[rng.random(Cf.shape) < 0.1] = np.inf
    Cf[1, 0] = -np.inf                     # infeasible under maximize
    Cf[2] = np.inf                         # every entry the best: value +inf, and feasible
    refs = [(c, -v) for c, v in refs_of(-Cf)]
    assert (refs[1][0] < 0).all() and refs[1][1] == -np.inf
    assert (refs[2][0] >= 0).all() and refs[2][1] == np.inf
    for C, (_, v) in zip(Cf, refs):  # the references' own maximize says the same
        assert lbap_ref(C, True)[1] == threshold_value(C, True) == v
    for tdt in (torch.float32, torch.float64, torch.bfloat16):
        check_against_refs(torch.from_numpy(Cf).to(tdt), refs, maximize=True)


# --------------------------------------------------------------------------- ragged and tall
@pytest.mark.parametrize("NR,NC", [(70, 70), (40, 300)])
@pytest.mark.parametrize("maximize", [False, True])
def test_ragged_batches_never_read_the_padding(NR, NC, maximize):
    rng = np.random.default_rng([14, NR, NC])
    shapes = np.array([[0, 3], [1, 1], [NR, NC], [NR // 2, NC - 1], [0, 0], [3, NC]], dtype=np.int32)
    B = len(shapes)
    live = rng.integers(-1000, 1000, size=(B, NR, NC))
    inside = (np.arange(NR)[None, :, None] < shapes[:, 0, None, None]) & \
             (np.arange(NC)[None, None, :] < shapes[:, 1, None, None])
    for dt in ("i64", "i32", "f64", "f32"):
        ndt = NUMPY[dt]
        if np.issubdtype(ndt, np.integer):
            poisons = [np.iinfo(ndt).max if maximize else np.iinfo(ndt).min]
        else:  # what would win if it were read, and NaN in a second run
            poisons = [np.inf if maximize else -np.inf, np.nan]
        refs = []
        for b, (r, c) in enumerate(shapes):
            col, value, _, _ = lbap_ref(live[b, :r, :c].astype(ndt), maximize)
            refs.append((np.concatenate([col, np.full(NR - r, -1, dtype=np.int32)]), value))
        for poison in poisons:
            Cb = np.where(inside, live, 0).astype(ndt)
            Cb[~inside] = poison
            check_against_refs(torch.from_numpy(Cb), refs, maximize=maximize, shapes=shapes)


@pytest.mark.parametrize("nr,nc", [(7, 3), (65, 64), (1025, 1000)])
def test_tall_input(nr, nc):
    rng = np.random.default_rng([15, nr, nc])
    Cb = rng.integers(0, 1 << 20, size=(2, nr, nc)).astype(np.float32)
    for b in range(2):
        col_t, rval, _, _ = lbap_ref(Cb[b].T)          # the row that each column takes
        want = np.full(nr, -1, dtype=np.int32)
        want[col_t] = np.arange(nc)
        for name, flags in designs(nr):
            col, value = solve(torch.from_numpy(Cb[b:b + 1]), flags)
            assert np.array_equal(col[0], want), name
            assert value.numpy()[0] == rval
            assert np.array_equal(np.sort(col[0][col[0] >= 0]), np.arange(nc))   # injective, onto all columns
            assert (col[0] < 0).sum() == nr - nc


# --------------------------------------------------------------------------- 4096
@functools.lru_cache(maxsize=None)
def large_cases():
    """Two 4096 x 4096 instances and one 2000 x 4096 (a ragged batch), integer
    valued below 2^24 so that float32 holds them exactly, and their thresholds."""
    rng = np.random.default_rng(16)
    Cb = rng.integers(0, 1 << 24, size=(3, 4096, 4096), dtype=np.int64)
    shapes = np.array([[4096, 4096], [4096, 4096], [2000, 4096]], dtype=np.int32)
    want = [threshold_value(Cb[b, :r, :c]) for b, (r, c) in enumerate(shapes)]
    return Cb, shapes, want


@pytest.mark.parametrize("dt", ["f32", "i64"])
def test_4096(dt):
    """The table has one configuration above 2048 columns, so there is no
    second one to compare col with; lbap_ref's loop is not run at this size."""
    Cb, shapes, want = large_cases()
    C = torch.from_numpy(Cb).to(TORCH[dt])
    col, value = solve(C, _lib.SH_FLAG_LBAP_MW, shapes=shapes)
    for b, (r, c) in enumerate(shapes):
        cb = col[b]
        assert (cb[r:] == -1).all()
        assert np.unique(cb[:r]).size == r and cb[:r].min() >= 0 and cb[:r].max() < c
        top = Cb[b, np.arange(r), cb[:r]].max()
        assert top == value.numpy()[b] == want[b], (b, top, value[b], want[b])


# --------------------------------------------------------------------------- front end, batch size
def test_front_end():
    rng = np.random.default_rng(17)
    for C in (rng.integers(-9, 9, size=(6, 8)), rng.integers(0, 2, size=(5, 5)).astype(bool),
              rng.integers(0, 200, size=(9, 4)).astype(np.uint8), rng.random((7, 7)).astype(np.float32),
              rng.random((12, 5)), rng.integers(0, 50, size=(4, 6)).astype(np.float16),
              rng.integers((1 << 63), (1 << 64) - 1, size=(5, 6), dtype=np.uint64)):
        for maximize in (False, True):
            rows, cols, value = linear_bottleneck_assignment(C, maximize=maximize)
            nr, nc = C.shape
            W = C.astype(np.float64) if C.dtype == np.uint64 else C.astype(np.int64) if C.dtype.kind in "bu" else C
            assert value.dtype == W.dtype
            if nr <= nc:
                rcol, rval, _, _ = lbap_ref(W, maximize)
                assert np.array_equal(rows, np.arange(nr)) and np.array_equal(cols, rcol)
            else:
                col_t, rval, _, _ = lbap_ref(W.T, maximize)
                order = np.argsort(col_t)
                assert np.array_equal(rows, col_t[order]) and np.array_equal(cols, order)
            assert rows.dtype == cols.dtype == np.int64
            chosen = W[rows, cols]
            assert value == rval == (chosen.min() if maximize else chosen.max())
    C = np.array([[1.0, np.inf], [2.0, np.inf]])
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        linear_bottleneck_assignment(C)
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        linear_bottleneck_assignment(-C.T, maximize=True)
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        linear_bottleneck_assignment(np.array([[1.0, np.nan], [2.0, 3.0]]))
    rows, cols, value = linear_bottleneck_assignment(np.array([[I64.min, I64.max], [I64.max, I64.max]]))
    assert value == I64.max and value.dtype == np.int64


def test_70000_instances_in_one_launch():
    """B beyond 65535 workgroups (the grid-size path), one wave each: every
    value against the exact optimum over all 8! permutations (a minimum over
    subsets of columns, row by row), a sample of 64 against the reference."""
    B, n = 70000, 8
    rng = np.random.default_rng(18)
    Cb = rng.integers(I32.min, I32.max, size=(B, n, n), endpoint=True).astype(np.int32)
    Cb[::3] = rng.integers(0, 4, size=Cb[::3].shape)
    col, value = solve(torch.from_numpy(Cb), _lib.SH_FLAG_LBAP_SW)
    value = value.numpy()
    best = np.full((B, 1 << n), I32.max, dtype=np.int32)   # best[b, S]: rows 0 .. |S| - 1 on the columns S
    best[:, 0] = I32.min
    for S in range(1, 1 << n):
        i = bin(S).count("1") - 1
        opts = [np.maximum(best[:, S ^ (1 << j)], Cb[:, i, j]) for j in range(n) if S >> j & 1]
        best[:, S] = np.minimum.reduce(opts)
    assert np.array_equal(value, best[:, -1])
    assert np.array_equal(np.sort(col, axis=1), np.broadcast_to(np.arange(n), (B, n)))
    assert np.array_equal(np.take_along_axis(Cb, col[:, :, None].astype(np.int64), 2).max(axis=(1, 2)), value)
    for b in rng.choice(B, size=64, replace=False):
        rcol, rval, _, _ = lbap_ref(Cb[b])
        assert np.array_equal(col[b], rcol) and value[b] == rval
