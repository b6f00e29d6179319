"""Free rows on the CSR on the GPU: every new entry against its
dense free-rows sibling on the densification (lsap.densify), entry by entry.
Equality is exact (integers, and the bits of every cost) everywhere except u,
v and theta, which are compared by value (a zero may carry the other sign; NaN
equals NaN).  Costs are integer-valued, so every sum is exact and the results
are also certified on the CSR itself: a perfect matching of the stored edges
(check_matching_sparse) at the cold sparse solve's cost.
"""
import functools

import numpy as np
import pytest
import torch

import free_rows_sparse_families as F
import santa_hip
from santa_hip import _lib, lsap

pytestmark = pytest.mark.gpu

DEV = "cuda"
STORAGE = {"f64": torch.float64, "f32": torch.float32}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bits(x):
    return x.contiguous().view(torch.int64)


def by_value(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


class Batch:
    """One CSR batch on the device with its densification (built once)."""

    def __init__(self, indptr, indices, data, shape, shapes, storage):
        self.shape, self.storage = tuple(shape), storage
        self.crow, self.idx = dev(indptr), dev(indices)
        self.val = dev(data, STORAGE[storage])
        self.shapes = None if shapes is None else np.asarray(shapes, dtype=np.int32)
        D = lsap.densify(indptr, indices, np.asarray(data, dtype=np.float64), self.shape)
        self.dense = dev(D.astype(np.float32) if storage == "f32" else D)
        self.corners = self.shapes if self.shapes is not None else np.tile(self.shape[1:], (self.shape[0], 1))

    def with_values(self, data):
        b = object.__new__(Batch)
        b.__dict__.update(self.__dict__)
        b.__dict__.pop("cold", None)   # (the cached cold solve is the other values')
        b.val = dev(data, STORAGE[self.storage])
        D = lsap.densify(self.crow, self.idx, np.asarray(data, dtype=np.float64), self.shape)
        b.dense = dev(D.astype(np.float32) if self.storage == "f32" else D)
        return b

    def sparse(self):
        return self.crow, self.idx, self.val, self.shape

    @functools.cached_property
    def cold(self):
        """(col, cost, u, v) of the cold sparse solve."""
        return santa_hip.solve_batched_sparse(*self.sparse(), shapes=self.shapes, duals=True)


def uniform(nr, nc, B, storage, density=0.05, shift=False):
    parts = [F.diag_random(nr, nc, s, density, shift) for s in range(B)]
    base = np.concatenate([[0], np.cumsum([p[1].size for p in parts])])
    indptr = np.concatenate([[0]] + [p[0][1:] + base[k] for k, p in enumerate(parts)]).astype(np.int64)
    return Batch(indptr, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), (B, nr, nc),
                 None, storage)


def of_family(insts, storage):
    b = F.batch(insts)
    data = np.where(np.isnan(b.data), 7.0, b.data)   # (entries beyond a corner: never read, but densify compares)
    return Batch(b.indptr, b.indices, data, b.shape, b.shapes, storage)


def redrawn(b, k, seed):
    """New values in k live rows of every instance, the pattern kept."""
    rng = np.random.default_rng([20261021, 37, k, seed])
    B, NR, NC = b.shape
    indptr = b.crow.cpu().numpy()
    data = b.val.double().cpu().numpy().copy()
    for q in range(B):
        live = int(b.corners[q][0])
        for i in rng.choice(live, size=min(k, live), replace=False):
            lo, hi = indptr[q * NR + i], indptr[q * NR + i + 1]
            data[lo:hi] = rng.integers(0, 1000, size=hi - lo)
    return b.with_values(data)


def check_warm(b, col0, v0, flags=0, maximize=False, certify=True, repeat=True):
    """resolve_batched_sparse_free_rows against resolve_batched_free_rows on the densification -> the result.
    repeat: run the sparse entry a second time and compare the bits."""
    B, NR, NC = b.shape
    u0 = torch.zeros((B, NR), dtype=torch.float64, device=DEV)
    keep = (col0.clone(), v0.clone(), b.val.clone())
    got = santa_hip.resolve_batched_sparse_free_rows(*b.sparse(), col0, u0, v0, flags=flags, shapes=b.shapes,
                                                     maximize=maximize)
    # (under maximize the dense entries' forbidden value is -inf)
    dense = torch.where(torch.isinf(b.dense), -b.dense, b.dense) if maximize else b.dense
    want = santa_hip.resolve_batched_free_rows(dense, col0, u0, v0, flags=flags, shapes=b.shapes, maximize=maximize)
    col, cost, u, v, kept, kept_free, theta = got
    dcol, dcost, du, dv, dkept, dkept_free, dtheta = want
    assert torch.equal(col, dcol), "col"
    assert torch.equal(kept, dkept) and torch.equal(kept_free, dkept_free), "kept"
    assert torch.equal(bits(cost), bits(dcost)), "cost bits"
    assert by_value(u, du) and by_value(v, dv) and by_value(theta, dtheta), "duals"
    # the search counts are the dense entry's
    live = torch.from_numpy(b.corners.astype(np.int64)).to(DEV)
    searches = (live[:, 0] - kept) + (live[:, 1] - live[:, 0] - kept_free)
    assert torch.equal(searches, (live[:, 0] - dkept) + (live[:, 1] - live[:, 0] - dkept_free))
    # inputs are not modified, and a second run gives equal bits
    assert torch.equal(col0, keep[0]) and torch.equal(bits(v0), bits(keep[1])) and torch.equal(b.val, keep[2])
    if repeat:
        again = santa_hip.resolve_batched_sparse_free_rows(*b.sparse(), col0, u0, v0, flags=flags, shapes=b.shapes,
                                                           maximize=maximize)
        for x, y in zip(got, again):
            assert torch.equal(x, y) if x.dtype == torch.int32 else torch.equal(bits(x), bits(y))
    if certify and not (flags & _lib.SH_FLAG_BUILD_ONLY) and not maximize:
        certify_result(b, col, cost)
    return got


def certify_result(b, col, cost):
    """A feasible result is a perfect matching of the stored edges at the cold sparse solve's cost; an infeasible
    one is exactly where the cold solve finds none."""
    ccol, ccost = b.cold[0], b.cold[1]
    B, NR, NC = b.shape
    feasible = torch.tensor([int(b.corners[q][0]) > 0 and int(ccol[q, 0]) >= 0 for q in range(B)], device=DEV)
    got_feasible = torch.tensor([int(b.corners[q][0]) > 0 and int(col[q, 0]) >= 0 for q in range(B)], device=DEV)
    assert torch.equal(feasible, got_feasible), "feasibility"
    assert torch.equal(bits(cost[feasible]), bits(ccost[feasible])), "the optimum"
    _, flags = santa_hip.check_matching_sparse(*b.sparse(), col, torch.zeros((B, NR), dtype=torch.uint8, device=DEV),
                                               shapes=b.shapes)
    assert not flags[feasible].any(), "not a perfect matching of the stored edges"


def states(b, small):
    """(name, col0, v0) from the cold solution of b."""
    B, NR, NC = b.shape
    col, _, _, v = b.cold
    rng = np.random.default_rng([20261021, 41, B, NR, NC])
    yield "solved", col, v
    yield "empty", torch.full_like(col, -1), torch.zeros_like(v)
    if small:   # anything: most virtual rows search as well
        gcol = dev(rng.integers(-3, NC + 3, size=(B, NR)).astype(np.int32))
        gv = np.where(rng.random((B, NC)) < 0.2, np.nan, rng.integers(-60, 20, size=(B, NC)).astype(np.float64))
        yield "garbage", gcol, dev(gv)
    else:       # garbage in eight rows and in 1 % of the duals: with nr of 1 or 3 a garbage v would make nearly every
        # virtual row search over up to NC tied columns (the fully garbage state: the test of its own below)
        gcol, gv = col.clone(), v.clone()
        rows = dev(rng.choice(NR, size=min(8, NR), replace=False))
        gcol[:, rows] = dev(rng.integers(-3, NC + 3, size=(B, rows.numel())).astype(np.int32))
        gv[:, dev(rng.choice(NC, size=max(1, NC // 100), replace=False))] = float("nan")
        yield "garbage", gcol, gv


# --------------------------------------------------------------------------- the warm start at every seam
SEAMS = (2, 5, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)
NR_OF = {"nc-1": lambda nc: nc - 1, "nc-7": lambda nc: nc - 7, "1": lambda nc: 1, "3": lambda nc: 3, "nc": lambda nc: nc}


def seam_cases():
    for nc in SEAMS:
        seen = set()
        for kind, f in NR_OF.items():
            nr = f(nc)
            if nr < 1 or nr > nc or nr in seen:
                continue
            seen.add(nr)
            for storage in STORAGE:
                yield pytest.param(nr, nc, storage, id=f"{nr}x{nc}-{storage}")


@pytest.mark.parametrize("nr,nc,storage", list(seam_cases()))
def test_warm_start_against_the_dense_free_rows_entry(nr, nc, storage):
    big = nc >= 2048
    b = uniform(nr, nc, 2 if big else 3, storage)
    if big and storage == "f64":   # the dense comparator holds float32 at these sizes
        b.dense = b.dense.float()
    col, _, _, v = b.cold
    for name, col0, v0 in states(b, small=nc <= 513):
        if name == "empty" and nc > 1025 and nr > 3:
            continue   # (a cold solve's worth of searches from the square state: the test below, one instance each)
        got = check_warm(b, col0, v0)
        if name == "solved":
            assert bool((got[4] == nr).all()) and bool((got[5] == nc - nr).all()) and torch.equal(got[0], col)
    for k in (1, 3):
        d = redrawn(b, k, nc)
        if big and storage == "f64":
            d.dense = d.dense.float()
        got = check_warm(d, col, v)
        assert bool((got[4] >= nr - k).all())
    if nr == nc:   # a square instance is resolve_batched_sparse's
        d = redrawn(b, 3, nc + 1)
        u0 = torch.zeros((b.shape[0], nr), dtype=torch.float64, device=DEV)
        got = santa_hip.resolve_batched_sparse_free_rows(*d.sparse(), col, u0, v)
        want = santa_hip.resolve_batched_sparse(*d.sparse(), col, u0, v)
        assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))
        assert by_value(got[2], want[2]) and by_value(got[3], want[3]) and torch.equal(got[4], want[4])
        assert not got[5].any() and by_value(got[6], got[3].max(dim=1).values)


def large_cases():
    for nc in (2048, 2049, 4096):
        for nr in (nc - 1, nc - 7, nc):
            for storage in STORAGE:
                yield pytest.param(nr, nc, storage, id=f"{nr}x{nc}-{storage}")


@pytest.mark.parametrize("nr,nc,storage", list(large_cases()))
def test_empty_state_on_the_eight_wave_kernels(nr, nc, storage):
    """Every real row searches from nothing in the (8, K, 12) continuations and displaces virtual rows: one
    instance, the float32 comparator, one run of each entry."""
    b = uniform(nr, nc, 1, storage)
    b.dense = b.dense.float()
    col, _, _, v = b.cold
    got = check_warm(b, torch.full_like(col, -1), torch.zeros_like(v), repeat=False)
    assert not got[4].any() and bool((got[5] == nc - nr).all())


# one fully garbage state per launch configuration above 513 columns, where the seam test's garbage state is the
# cold solution with eight garbage rows: (4, 4, 10), (8, 4, 12), (8, 6, 12), (8, 8, 12).  nr = nc - 7: with few real
# rows nearly every virtual row would search, each over up to nc tied columns
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("nc", (1024, 2048, 2049, 4096))
def test_garbage_state_on_every_large_configuration(nc, storage):
    nr = nc - 7
    b = uniform(nr, nc, 1, storage)
    b.dense = b.dense.float()
    rng = np.random.default_rng([20261021, 47, nc])
    gcol = dev(rng.integers(-3, nc + 3, size=(1, nr)).astype(np.int32))
    gv = np.where(rng.random((1, nc)) < 0.2, np.nan, rng.integers(-60, 20, size=(1, nc)).astype(np.float64))
    check_warm(b, gcol, dev(gv), repeat=False)


def family_batches():
    fam = F.family()
    for at in range(0, len(fam), 3):
        for storage in STORAGE:
            yield pytest.param(fam[at:at + 3], storage, id=f"{fam[at].name}-{storage}")


@pytest.mark.parametrize("insts,storage", list(family_batches()))
def test_warm_start_on_the_families_ragged(insts, storage):
    b = of_family(insts, storage)
    B, NR, NC = b.shape
    for seed in range(2):
        per = [{s[0]: s[1:] for s in F.states(g, seed)} for g in insts]
        for name in ("solved", "dropped", "garbage", "empty"):
            col0 = -np.ones((B, NR), dtype=np.int32)
            v0 = np.zeros((B, NC))
            for q, (g, st) in enumerate(zip(insts, per)):
                c, v = st.get(name, st["garbage"])
                col0[q, :g.shape[0]], v0[q, :g.shape[1]] = c, v
            check_warm(b, dev(col0), dev(v0))
            check_warm(b, dev(col0), dev(v0), flags=_lib.SH_FLAG_BUILD_ONLY)
            if not np.isinf(b.val.cpu().numpy()).any():   # (a stored +inf under maximize is the caller's to reject)
                check_warm(b, dev(col0), dev(-v0), maximize=True)


def test_infeasible_instances_answer_as_the_dense_entry():
    insts = [g for g in F.family() if g.name in ("hall", "empty_row", "hall_wide")]
    assert len(insts) == 3
    b = of_family(insts, "f64")
    B, NR, NC = b.shape
    got = check_warm(b, torch.zeros((B, NR), dtype=torch.int32, device=DEV), torch.zeros((B, NC), dtype=torch.float64,
                                                                                         device=DEV))
    col, cost, u, v, kept, kept_free, theta = got
    assert bool((col == -1).all()) and not cost.any() and bool(torch.isnan(theta).all())
    for q, g in enumerate(insts):
        nr, nc = g.corner
        assert bool(torch.isnan(u[q, :nr]).all()) and bool(torch.isnan(v[q, :nc]).all())
        assert not u[q, nr:].any() and not v[q, nc:].any()


def test_build_only_leaves_the_start_state_at_a_multi_wave_size():
    b = uniform(250, 257, 2, "f64")
    col, _, _, v = b.cold
    d = redrawn(b, 3, 5)
    got = check_warm(d, col, v, flags=_lib.SH_FLAG_BUILD_ONLY)
    assert bool((got[4] >= 247).all()) and bool((got[5] == 7).all()) and not got[1].any()
    assert torch.equal(bits(got[3]), bits(v))   # no dual is raised
    check_warm(d, col, -v, maximize=True)


def test_single_matrix_front_end_on_one_wide_matrix():
    indptr, indices, data = F.diag_random(60, 67, 9, 0.2)
    A = (indptr, indices, data, (60, 67))
    rows, col, u, v = santa_hip.linear_sum_assignment_sparse(A, duals=True)
    data2 = data.copy()
    data2[indptr[7]:indptr[8]] = 999 - data2[indptr[7]:indptr[8]]
    A2 = (indptr, indices, data2, (60, 67))
    r2, c2, u2, v2 = santa_hip.linear_sum_assignment_sparse_resolve(A2, col, u, v, free_rows=True)
    D = lsap.densify(indptr, indices, data2, (60, 67))
    cold = santa_hip.linear_sum_assignment_sparse(A2)
    assert np.array_equal(r2, np.arange(60)) and np.unique(c2).size == 60
    assert D[r2, c2].sum() == D[cold[0], cold[1]].sum()
    dense = santa_hip.linear_sum_assignment_resolve(D, col, u, v, free_rows=True)
    assert np.array_equal(dense[1], c2) and np.array_equal(dense[2], u2) and np.array_equal(dense[3], v2)


# --------------------------------------------------------------------------- Murty's children
def forb_sets(b, p):
    """F of row p: empty, one bit, bits 63 and 64, all stored columns of row p (int64 words [B, W])."""
    B, NR, NC = b.shape
    W = lsap.forbidden_words(NC)
    indptr, idx = b.crow.cpu().numpy(), b.idx.cpu().numpy()

    def words(cols_of):
        F_ = np.zeros((B, W), dtype=np.uint64)
        for q in range(B):
            for j in cols_of(q):
                F_[q, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
        return dev(F_.view(np.int64))

    yield "empty", words(lambda q: [])
    yield "one", words(lambda q: [int(idx[indptr[q * NR + p]])])
    if NC > 64:
        yield "63_64", words(lambda q: [63, 64])
    yield "row", words(lambda q: [int(j) for j in idx[indptr[q * NR + p]:indptr[q * NR + p + 1]]])


def check_children(b, col, v, p, forb):
    got = santa_hip.murty_children_batched_sparse(*b.sparse(), col, v, p, forb, shapes=b.shapes, free_rows=True)
    want = santa_hip.murty_children_batched(b.dense, col, v, p, forb, shapes=b.shapes, free_rows=True)
    assert torch.equal(got[0], want[0]), "col"
    assert torch.equal(bits(got[1]), bits(want[1])), "cost bits"
    assert by_value(got[2], want[2]) and by_value(got[3], want[3]), "duals"
    assert torch.equal(got[4], want[4]), "kept"
    return got


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("wide", (False, True), ids=("square", "nc-3"))
@pytest.mark.parametrize("nc", (5, 64, 65, 256, 257, 512, 513, 1024))
def test_children_against_the_dense_free_rows_children(nc, wide, storage):
    nr = nc - 3 if wide else nc
    b = uniform(nr, nc, 1 if nc > 513 else 2, storage, density=0.08, shift=True)
    B = b.shape[0]
    col, _, _, v = b.cold
    assert bool((col >= 0).all())
    some = 0   # (child 0 of the root exists: the pattern holds two matchings that differ in row 0)
    for p in sorted({0, nr // 2, nr - 1}):
        pt = torch.full((B,), p, dtype=torch.int32, device=DEV)
        for name, forb in forb_sets(b, p):
            got = check_children(b, col, v, pt, forb)
            some += int(torch.isfinite(got[1]).sum())
    assert some > 0
    # the node as garbage data
    rng = np.random.default_rng([nc, nr, 43])
    gcol = dev(rng.integers(-2, nc + 2, size=(B, nr)).astype(np.int32))
    gv = dev(np.where(rng.random((B, nc)) < 0.1, np.nan, rng.integers(-50, 10, size=(B, nc)).astype(np.float64)))
    gp = dev(rng.integers(-1, nr, size=B).astype(np.int32))
    gf = dev(rng.integers(-(1 << 62), 1 << 62, size=(B, lsap.forbidden_words(nc)), dtype=np.int64))
    check_children(b, gcol, gv, gp, gf)


# --------------------------------------------------------------------------- the k best
def check_kbest(b, k, integer_valued=True):
    got = santa_hip.kbest_batched_sparse(*b.sparse(), k=k, shapes=b.shapes, free_rows=True)
    want = santa_hip.kbest_batched(b.dense, k, shapes=b.shapes, free_rows=True)
    assert torch.equal(got[0], want[0]), "cols"
    assert torch.equal(bits(got[1]), bits(want[1])), "costs bits"
    assert torch.equal(got[2], want[2]), "count"
    if integer_valued:   # the default mode's costs
        plain = santa_hip.kbest_batched_sparse(*b.sparse(), k=k, shapes=b.shapes)
        assert torch.equal(bits(got[1]), bits(plain[1])) and torch.equal(got[2], plain[2])
    return got


@pytest.mark.parametrize("insts,storage", list(family_batches()))
def test_kbest_on_the_families_ragged(insts, storage):
    b = of_family(insts, storage)
    check_kbest(b, 12)
    if np.isinf(b.val.cpu().numpy()).any():
        return   # (a stored +inf under maximize is the caller's to reject)
    got = santa_hip.kbest_batched_sparse(*b.sparse(), k=12, shapes=b.shapes, maximize=True, free_rows=True)
    want = santa_hip.kbest_batched(torch.where(torch.isinf(b.dense), -b.dense, b.dense), 12, shapes=b.shapes,
                                   maximize=True, free_rows=True)
    assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1])) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("nr,nc", ((60, 67), (250, 257)))
def test_kbest_at_multi_wave_sizes(nr, nc, storage):
    b = uniform(nr, nc, 2, storage, density=0.1)
    cols, costs, count = check_kbest(b, 3)
    assert bool((count == 3).all()) and bool((costs[:, 1:] >= costs[:, :-1]).all())
    # k = 1 is the cold sparse solve
    one = santa_hip.kbest_batched_sparse(*b.sparse(), k=1, free_rows=True)
    assert torch.equal(one[0][:, 0], b.cold[0]) and torch.equal(bits(one[1][:, 0]), bits(b.cold[1]))
    assert torch.equal(cols[:, 0], b.cold[0])


def test_kbest_of_an_infeasible_root():
    insts = [g for g in F.family() if g.name in ("hall", "hall_wide", "all_and_none")]
    b = of_family(insts, "f64")
    cols, costs, count = check_kbest(b, 4)
    by_name = {g.name: q for q, g in enumerate(insts)}
    for name in ("hall", "hall_wide"):
        q = by_name[name]
        assert int(count[q]) == 0 and bool((cols[q] == -1).all()) and bool(torch.isinf(costs[q]).all())
    assert int(count[by_name["all_and_none"]]) == 4


def test_kbest_assignments_sparse_with_free_rows():
    indptr, indices, data = F.diag_random(20, 27, 3, 0.3)
    D = lsap.densify(indptr, indices, data, (20, 27))
    try:
        import scipy.sparse as sp
        A = sp.csr_matrix((data, indices, indptr), shape=(20, 27))
    except ImportError:
        A = (indptr, indices, data, (20, 27))
    cols, costs = santa_hip.kbest_assignments_sparse(A, 5, free_rows=True)
    want_cols, want_costs = santa_hip.kbest_assignments(D, 5, free_rows=True)
    assert np.array_equal(cols, want_cols) and np.array_equal(costs, want_costs)
    plain = santa_hip.kbest_assignments_sparse(A, 5)
    assert np.array_equal(costs, plain[1])
    assert np.array_equal(D[np.arange(20)[:, None], cols.T].sum(axis=0), costs)
