"""GPU tests of check_duals_sparse (the lsap_check_duals_csr_ entries): slack
and flags are bit for bit those of check_duals_large on the densification
(existing code, not code under test) and those of the host reference
(lsap_csr_cert_ref), on every sparse family at the seams of the layout, on
planted faults and on the rule for duals that are not finite."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_cert_ref as C  # noqa: E402
import lsap_sparse_families as S  # noqa: E402
from lsap_csr_cert_ref import csr_cert_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (3, 5), (64, 64), (63, 65), (40, 129), (300, 300), (60, 1025), (40, 4096))
CASES = [(f, nr, nc) for f, nr, nc in S.cases() if (nr, nc) in SHAPES]


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    for name in ("check_duals_sparse", "solve_batched_sparse", "check_duals_large"):
        assert hasattr(santa_hip, name), f"santa_hip has no {name}"
    return santa_hip


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def reference(indptr, indices, data, nr, nc, col, u, v, shapes=None):
    """csr_cert_ref of every instance of a batch -> (slack [B, 3], flags [B])."""
    B = col.shape[0]
    out = [csr_cert_ref(indptr[k * nr:(k + 1) * nr + 1], indices, data, nr, nc, col[k], u[k], v[k],
                        None if shapes is None else shapes[k]) for k in range(B)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def dense_check(sh, indptr, indices, data, nr, nc, col, u, v, shapes=None):
    """check_duals_large on the densification -> (slack [B, 3], flags [B]) on the host."""
    B = col.shape[0]
    D = sh.densify(indptr, indices, data, (B, nr, nc))
    D[np.isnan(D)] = 7.0  # (NaN lies outside the corners only, where nothing is read)
    s0, s1, s2, fl = sh.check_duals_large(dev(D), dev(col), dev(u), dev(v), shapes=shapes)
    return torch.stack([s0, s1, s2], dim=1).cpu().numpy(), fl.cpu().numpy()


def sparse_check(sh, indptr, indices, data, nr, nc, col, u, v, shapes=None, dtype=torch.float64, **kw):
    B = col.shape[0]
    slack, fl = sh.check_duals_sparse(dev(indptr), dev(indices), dev(data, dtype), (B, nr, nc), dev(col), dev(u), dev(v),
                                      shapes=shapes, **kw)
    assert slack.dtype == torch.float64 and tuple(slack.shape) == (B, 3)
    assert fl.dtype == torch.int32 and tuple(fl.shape) == (B,)
    return slack.cpu().numpy(), fl.cpu().numpy()


def assert_all_equal(sh, indptr, indices, data, nr, nc, col, u, v, shapes=None):
    """The sparse certificate against the dense one and the reference; returns it."""
    slack, fl = sparse_check(sh, indptr, indices, data, nr, nc, col, u, v, shapes)
    want_s, want_f = reference(indptr, indices, data, nr, nc, col, u, v, shapes)
    print("sparse", slack.tolist(), fl.tolist(), "reference", want_s.tolist(), want_f.tolist())
    assert np.array_equal(fl, want_f) and C.same_bits(slack, want_s), "differs from the host reference"
    dslack, dfl = dense_check(sh, indptr, indices, data, nr, nc, col, u, v, shapes)
    assert np.array_equal(fl, dfl) and C.same_bits(slack, dslack), "differs from check_duals_large on the densification"
    return slack, fl


def solved(sh, b, nr, nc, shapes=None, **kw):
    B = len(b.dense)
    col, _, u, v = sh.solve_batched_sparse(dev(b.indptr), dev(b.indices), dev(b.data), shape=(B, nr, nc), shapes=shapes,
                                           duals=True, **kw)
    return col.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("family,nr,nc", CASES)
def test_families_certify_as_their_densification(sh, family, nr, nc):
    b = S.batch(family, nr, nc)
    shapes = np.array(b.corners, dtype=np.int32) if b.corners else None
    col, u, v = solved(sh, b, nr, nc, shapes)
    slack, fl = assert_all_equal(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v, shapes)
    for k, D in enumerate(b.dense):
        assert fl[k] == (0 if b.feasible[k] or D.shape[0] == 0 else C.NONE), k
    s32, f32 = sparse_check(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v, shapes, dtype=torch.float32)
    assert np.array_equal(f32, fl) and C.same_bits(s32, slack), "float32 storage of values that are exact in it"


def random_batch(nr, nc, B, p, seed):
    rng = np.random.default_rng(seed)
    P = (rng.random((B * nr, nc)) < p)
    P[np.arange(B * nr), np.tile(np.arange(nr), B)] = True
    return S.csr_of(P, rng.random((B * nr, nc)) * 100 - 30)


def test_gap_summation_order_shows_on_random_values(sh):
    nr = nc = 300
    indptr, indices, data = random_batch(nr, nc, 4, 0.3, 11)
    b = S.Batch(indptr, indices, data, [np.empty((nr, nc))] * 4, None, None)
    col, u, v = solved(sh, b, nr, nc)
    slack, fl = assert_all_equal(sh, indptr, indices, data, nr, nc, col, u, v)
    assert not (fl & ~(C.SLACK | C.TIGHT)).any()   # (float duals are feasible up to rounding only)
    # the order matters at this size: another order of the waves gives other bits somewhere
    other = [C.ordered_sum(u[k], np.arange(nr), waves=(3, 2, 1, 0)) for k in range(4)]
    assert any(o != C.ordered_sum(u[k], np.arange(nr)) for k, o in enumerate(other))
    # float32 values: widened exactly, certified as the float64 matrix that holds them
    d32 = data.astype(np.float32)
    s32, f32 = sparse_check(sh, indptr, indices, d32, nr, nc, col, u, v, dtype=torch.float32)
    want_s, want_f = reference(indptr, indices, d32, nr, nc, col, u, v)
    assert np.array_equal(f32, want_f) and C.same_bits(s32, want_s)


@pytest.fixture(scope="module")
def base(sh):
    """One solved batch for the planted faults: band_40pct at (40, 129), 8 instances."""
    nr, nc = 40, 129
    b = S.batch("band_40pct", nr, nc)
    col, u, v = solved(sh, b, nr, nc)
    assert (col >= 0).all()
    return b, nr, nc, col, u, v


def entry_of(b, nr, k, i, j):
    """The index in data of the stored entry (k, i, j)."""
    e0, e1 = b.indptr[k * nr + i], b.indptr[k * nr + i + 1]
    at = np.flatnonzero(b.indices[e0:e1] == j)
    assert at.size == 1
    return int(e0 + at[0])


def test_an_entry_below_its_dual_sum_is_found_wherever_it_sits(sh, base):
    b, nr, nc, col, u, v = base
    data = b.data.copy()
    plants = []
    for k, (i, where) in enumerate([(0, "first"), (0, "last"), (nr - 1, "first"), (nr - 1, "last"), (7, 63), (7, 64),
                                    (nr - 1, 128), (0, 0)]):
        e0, e1 = b.indptr[k * nr + i], b.indptr[k * nr + i + 1]
        if where == "first":
            e = e0
        elif where == "last":
            e = e1 - 1
        else:  # the stored entry of the row at or after the column, in its 64-column word if there is one
            cand = [e for e in range(e0, e1) if b.indices[e] % 64 == where % 64]
            e = cand[0] if cand else e0
        j = int(b.indices[e])
        data[e] = u[k, i] + v[k, j] - 3.0 - k
        plants.append((k, i, j, data[e]))
    slack, fl = assert_all_equal(sh, b.indptr, b.indices, data, nr, nc, col, u, v)
    for k, i, j, val in plants:
        assert fl[k] & C.SLACK and slack[k, 0] == (val - u[k, i]) - v[k, j] and slack[k, 0] <= -3.0, (k, i, j)


def test_chosen_entries_raised_or_removed_are_not_tight(sh, base):
    b, nr, nc, col, u, v = base
    data = b.data.copy()
    keep = np.ones(data.size, dtype=bool)
    for k in range(8):
        i = (5 * k) % nr
        e = entry_of(b, nr, k, i, col[k, i])
        if k % 2:
            keep[e] = False       # removed from the CSR: the pair is missing
        else:
            data[e] += 2.0        # raised
    indptr = np.concatenate([[0], np.cumsum(keep)])[b.indptr]
    slack, fl = assert_all_equal(sh, indptr, b.indices[keep], data[keep], nr, nc, col, u, v)
    for k in range(8):
        assert fl[k] == C.TIGHT, (k, fl[k])
        assert slack[k, 1] == (np.inf if k % 2 else 2.0)
        assert slack[k, 2] == (-np.inf if k % 2 else -2.0)


def test_bad_col_and_signs(sh, base):
    b, nr, nc, col, u, v = base
    col, v = col.copy(), v.copy()
    col[0, 3] = col[0, 4]           # a duplicate
    col[1, nr - 1] = nc             # out of range
    col[2, 0] = -1                  # a live row without a column next to rows with
    col[3, 5] = -7
    col[4, 1] = np.iinfo(np.int32).max
    free = sorted(set(range(nc)) - set(col[5].tolist()))
    v[5, free[0]] = 1.0             # v > 0
    v[6, free[-1]] = -1.0           # v != 0 on a column no row took
    slack, fl = assert_all_equal(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v)
    assert all(fl[k] & C.COL for k in range(5)) and fl[5] & C.SIGN and fl[6] & C.SIGN and fl[7] == 0
    # every row without a column: nothing is certified
    none = np.full_like(col, -1)
    slack, fl = assert_all_equal(sh, b.indptr, b.indices, b.data, nr, nc, none, u, v)
    assert (fl == C.NONE).all() and not slack.any()


def test_duals_that_are_not_finite(sh, base):
    """The added rule: slack[0] is NaN and SLACK is set; checked against the
    reference (the dense certificate has no missing entries to be undefined on)."""
    b, nr, nc, col, u, v = base
    u, v = u.copy(), v.copy()
    u[0, 0], u[1, nr - 1], u[2, 5] = np.inf, -np.inf, np.nan
    v[3, 0], v[4, nc - 1], v[5, 64] = -np.inf, np.nan, np.inf
    slack, fl = sparse_check(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v)
    want_s, want_f = reference(b.indptr, b.indices, b.data, nr, nc, col, u, v)
    print(slack.tolist(), fl.tolist(), want_s.tolist(), want_f.tolist())
    assert np.array_equal(fl, want_f) and C.same_bits(slack, want_s)
    assert np.isnan(slack[:6, 0]).all() and (fl[:6] & C.SLACK).all() and fl[6] == 0 and fl[7] == 0
    # outside the live corner a dual is not read
    shapes = np.tile(np.array([[nr - 1, nc - 1]], dtype=np.int32), (8, 1))
    u2, v2 = np.zeros_like(u), np.zeros_like(v)
    u2[:, nr - 1], v2[:, nc - 1] = np.nan, np.inf
    col2 = np.full_like(col, -1)
    col2[:, 0] = 0
    slack, fl = assert_all_equal(sh, b.indptr, b.indices, b.data, nr, nc, col2, u2, v2, shapes)
    assert not np.isnan(slack).any()


@pytest.mark.parametrize("family,nr,nc", [("band_5pct", 64, 64), ("explicit_zero", 40, 129), ("hall", 63, 65)])
def test_maximize_certifies_the_negated_problem(sh, family, nr, nc):
    b = S.batch(family, nr, nc)
    B = len(b.dense)
    col, u, v = solved(sh, b, nr, nc, maximize=True)
    slack, fl = sparse_check(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v, maximize=True)
    want_s, want_f = reference(b.indptr, b.indices, -b.data, nr, nc, col, -u, -v)
    assert np.array_equal(fl, want_f) and C.same_bits(slack, want_s)
    assert (fl == (C.NONE if family == "hall" else 0)).all()
    D = sh.densify(b.indptr, b.indices, b.data, (B, nr, nc))
    D[np.isinf(D)] = -np.inf  # (the forbidden value of a problem to maximise)
    s0, s1, s2, dfl = sh.check_duals_large(dev(D), dev(col), dev(u), dev(v), maximize=True)
    assert np.array_equal(dfl.cpu().numpy(), fl) and C.same_bits(torch.stack([s0, s1, s2], 1).cpu().numpy(), slack)


def test_indices_outside_the_matrix_are_no_entries(sh, base):
    """validate=False: an index outside [0, nc) is read as data and dropped; the
    result is that of the matrix without those entries."""
    b, nr, nc, col, u, v = base
    rows = 8 * nr
    extra_lo, extra_hi = np.arange(rows) % 3 == 0, np.arange(rows) % 2 == 0   # one before, one or two after
    idx, val, ptr = [], [], [0]
    for r in range(rows):
        e0, e1 = b.indptr[r], b.indptr[r + 1]
        lo = [-1 - r] if extra_lo[r] else []
        hi = [nc, np.iinfo(np.int32).max] if extra_hi[r] else [nc + 5]
        idx += lo + b.indices[e0:e1].tolist() + hi
        val += [np.nan] * len(lo) + b.data[e0:e1].tolist() + [-1e300] * len(hi)
        ptr.append(len(idx))
    slack, fl = sparse_check(sh, np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int32), np.array(val), nr, nc,
                             col, u, v, validate=False)
    clean_s, clean_f = sparse_check(sh, b.indptr, b.indices, b.data, nr, nc, col, u, v)
    assert np.array_equal(fl, clean_f) and C.same_bits(slack, clean_s) and not fl.any()
