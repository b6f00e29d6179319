"""The bottleneck solver's witness (lbap_solve_wit_) and its certificate
(lbap_check_) on the GPU.  Up to 257 columns col, value and wit are array-equal
to the host loop (lbap_witness_ref) in every design, no tolerance; at the seams
of the launch table and above, where the loop is too slow, the closed-form
families of lbap_cert_families.py and, on a random instance, the certificate
itself (lbap_check_ref on the GPU's output: flags == 0 is a proof).
check_bottleneck equals lbap_check_ref on the solver's output, on every
mutation proved in test_lbap_cert_cpu.py and on malformed input."""
import functools

import numpy as np
import pytest
import torch

import lbap_cert_families as F
from lbap_cert_ref import SH_LBCERT_NONE, lbap_check_ref, lbap_witness_ref
from santa_hip import _lib, check_bottleneck, linear_bottleneck_assignment, solve_bottleneck_batched
from test_lbap_gpu import designs, to_host

pytestmark = pytest.mark.gpu


def to_torch(S, dt):
    S = np.ascontiguousarray(S)
    return torch.from_numpy(S.view(np.int16)).view(torch.bfloat16) if dt == "bf16" else torch.from_numpy(S)


def solve_wit(C, flags=0, **kw):
    col, value, wit = solve_bottleneck_batched(C, flags=flags, witness=True, **kw)
    torch.cuda.synchronize()
    return col.cpu().numpy(), value, wit.cpu().numpy()


def check(C, col, value, wit, **kw):
    """check_bottleneck -> int arrays [B, 3] = (nR, nN, flags)."""
    out = check_bottleneck(C, torch.as_tensor(col).cuda(), value.cuda(), torch.as_tensor(wit).cuda(), **kw)
    torch.cuda.synchronize()
    return np.stack([x.cpu().numpy() for x in out], axis=1)


# --------------------------------------------------------------------------- up to 257 columns
@functools.lru_cache(maxsize=None)
def small_batch(nr, nc, maximize, flt):
    """(V [B, nr, nc] int64 or float64 values exact in every dtype, shapes,
    refs): ties, a ragged member, an empty one, tie_no_rewrite; floats: about
    half the entries forbidden around a finite permutation, and that with one
    row forbidden throughout (infeasible).  One reference for all dtypes."""
    rng = np.random.default_rng([31, nr, nc, maximize])
    M = [rng.integers(-3, 4, size=(nr, nc)), rng.integers(-128, 129, size=(nr - 3, nc - 2)),
         np.zeros((0, nc), dtype=np.int64), F.tie_no_rewrite(nr, nc)]
    if flt:
        forb = -np.inf if maximize else np.inf
        P = rng.integers(-3, 4, size=(nr, nc)).astype(np.float64)
        keep = rng.random((nr, nc)) < 0.5
        keep[np.arange(nr), rng.permutation(nc)[:nr]] = True
        P[~keep] = forb
        Q = P.copy()
        Q[nr // 2] = forb
        M = [m.astype(np.float64) for m in M] + [P, Q]
    V = np.zeros((len(M), nr, nc), dtype=np.float64 if flt else np.int64)
    V[:] = (np.inf if maximize else -np.inf) if flt else (127 if maximize else -128)  # what would win if read
    refs = []
    for b, m in enumerate(M):
        V[b, :m.shape[0], :m.shape[1]] = m
        col, value, wit = lbap_witness_ref(m, maximize)
        pad = nr - m.shape[0]
        refs.append((np.concatenate([col, np.full(pad, -1, np.int32)]), value, np.concatenate([wit, np.zeros(pad, np.uint8)])))
    return V, np.array([m.shape for m in M], dtype=np.int32), refs


@pytest.mark.parametrize("maximize", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("nr,nc", F.SMALL_SHAPES)
@pytest.mark.parametrize("dt", F.DTYPES)
def test_witness_equals_the_host_loop_in_every_design(dt, nr, nc, maximize):
    V, shapes, refs = small_batch(nr, nc, maximize, dt in F.FLOATS)
    S = F.store(V, dt)
    assert np.array_equal(F.widen(S, dt), V)
    C = to_torch(S, dt).cuda()
    for name, flags in designs(nc):
        col, value, wit = solve_wit(C, flags, maximize=maximize, shapes=shapes)
        col0, value0 = solve_bottleneck_batched(C, flags=flags, maximize=maximize, shapes=shapes)
        assert np.array_equal(col, col0.cpu().numpy()) and torch.equal(value.view(torch.uint8), value0.view(torch.uint8))
        v = to_host(value)
        for b, (rcol, rval, rwit) in enumerate(refs):
            assert np.array_equal(col[b], rcol), (name, b)
            assert v[b] == rval, (name, b, v[b], rval)
            assert np.array_equal(wit[b], rwit), (name, b, np.flatnonzero(wit[b] != rwit)[:8])
    # the certificate of the last design's output: lbap_check_ref's counts and flags, and the proof itself
    got = check(C, col, value, wit, maximize=maximize, shapes=shapes)
    for b, (r, c) in enumerate(shapes):
        want = lbap_check_ref(V[b], col[b], v[b], wit[b], maximize, shape=(r, c))
        assert tuple(got[b]) == want, (b, got[b], want)
        infeasible = r > 0 and (refs[b][0][:r] < 0).all()
        assert got[b, 2] == (SH_LBCERT_NONE if infeasible else 0)
        assert got[b, 1] == got[b, 0] - 1 or r == 0


@pytest.mark.parametrize("nr,nc", [(40, 60), (130, 256)])
def test_maximize_over_the_whole_int64_range_ragged(nr, nc):
    M = [F.maximize_full_range(nr, nc, 0), F.maximize_full_range(nr - 7, nc - 1, 1), F.maximize_full_range(1, nc, 2)]
    V = np.full((3, nr, nc), F.I64.max, dtype=np.int64)
    for b, m in enumerate(M):
        V[b, :m.shape[0], :m.shape[1]] = m
    shapes = np.array([m.shape for m in M], dtype=np.int32)
    C = torch.from_numpy(V).cuda()
    for name, flags in designs(nc):
        col, value, wit = solve_wit(C, flags, maximize=True, shapes=shapes)
        for b, m in enumerate(M):
            rcol, rval, rwit = lbap_witness_ref(m, True)
            r = m.shape[0]
            assert np.array_equal(col[b, :r], rcol) and (col[b, r:] == -1).all(), (name, b)
            assert value[b].item() == rval and np.array_equal(wit[b, :r], rwit) and not wit[b, r:].any(), (name, b)
    got = check(C, col, value, wit, maximize=True, shapes=shapes)
    assert not got[:, 2].any() and (got[:, 1] == got[:, 0] - 1).all()
    assert check(C, col, value, wit, maximize=False, shapes=shapes)[:, 2].all()  # the other order refuses it


@pytest.mark.parametrize("dt", ["i32", "f32"])
def test_tall_batches_mark_columns(dt):
    nr, nc = 130, 60
    V = np.stack([np.random.default_rng([32, k]).integers(-3, 4, size=(nr, nc)) for k in range(2)])
    C = to_torch(F.store(V, dt), dt).cuda()
    for name, flags in designs(nr):   # (the transposed batch has nr columns)
        col, value, wit = solve_wit(C, flags, maximize=True)
        assert wit.shape == (2, nc)
        for b in range(2):
            col_t, rval, rwit = lbap_witness_ref(V[b].T, True)   # the row that each column takes
            w = np.full(nr, -1, dtype=np.int32)
            w[col_t] = np.arange(nc)
            assert np.array_equal(col[b], w) and to_host(value)[b] == rval and np.array_equal(wit[b], rwit), (name, b)
    got = check(C, col, value, wit, maximize=True)
    for b in range(2):
        col_t = np.full(nc, -1)
        col_t[col[b][col[b] >= 0]] = np.flatnonzero(col[b] >= 0)
        assert tuple(got[b]) == lbap_check_ref(V[b].T, col_t, to_host(value)[b], wit[b], True) and got[b, 2] == 0
    bad = col.copy()
    bad[0, 0] = bad[0, 1] = 5   # no assignment before its inversion
    assert check(C, bad, value, wit, maximize=True)[0, 2] & _lib.SH_LBCERT_COL


# --------------------------------------------------------------------------- the seams and above
SEAMS = [(dt, n, 0) for dt in F.DTYPES for n in F.SEAM_SIZES[dt]] + [(dt, F.SW_SEAM, F.SH_FLAG_LBAP_SW) for dt in F.DTYPES]


@pytest.mark.parametrize("dt,n,flags", SEAMS, ids=lambda x: str(x))
def test_closed_forms_at_the_seams(dt, n, flags):
    members = F.seam_members(dt, n)
    flt = dt in F.FLOATS
    V = [F.build(family, n, n, k).astype(np.float64 if flt else np.int64) for family, k in members]
    rnd = dt in ("f32", "i64") and not flags   # one random instance per size: the certificate is its proof
    if rnd:
        V.append(np.random.default_rng([33, n]).integers(0, 1 << 20, size=(n, n)).astype(V[0].dtype))
    V = np.stack(V)
    S = F.store(V, dt)
    del V
    C = to_torch(S, dt).cuda()
    col, value, wit = solve_wit(C, flags)
    v = to_host(value)
    for b, (family, k) in enumerate(members):
        wcol, wval, wwit = F.closed_form(family, n, n, k)
        assert np.array_equal(col[b], wcol) and v[b] == wval, (family, v[b], wval)
        assert np.array_equal(wit[b], wwit), (family, int(wit[b].sum()), int(wwit.sum()))
    got = check(C, col, value, wit)
    for b, (family, k) in enumerate(members):
        nR = int(F.closed_form(family, n, n, k)[2].sum())
        assert tuple(got[b]) == (nR, nR - 1, SH_LBCERT_NONE if family == "infeasible_hall" else 0), (family, got[b])
    if rnd:
        b = len(members)
        want = lbap_check_ref(F.widen(S[b], dt), col[b], v[b], wit[b])
        assert want[2] == 0 and want[1] == want[0] - 1, want   # optimal, proved on the host without the loop
        assert tuple(got[b]) == want


# --------------------------------------------------------------------------- check_bottleneck
def test_check_equals_the_reference_on_every_mutation():
    for name, C, col, value, wit, maximize, bit in F.mutation_cases():
        Ct = torch.from_numpy(C[None]).cuda()
        got = check(Ct, col[None].astype(np.int32), torch.from_numpy(np.array([value], dtype=C.dtype)), wit[None],
                    maximize=maximize)
        want = lbap_check_ref(C, col, value, wit, maximize)
        assert tuple(got[0]) == want and got[0, 2] & bit, (name, got[0], want)


def test_malformed_col_and_wit_are_flagged_not_followed():
    """col far outside [-1, nc), wit bytes other than 0 / 1, a padded row with a
    column: flags and counts as lbap_check_ref gives them, and nothing faults."""
    rng = np.random.default_rng(34)
    NR, NC = 70, 300
    V = rng.integers(-50, 50, size=(6, NR, NC)).astype(np.int32)
    shapes = np.array([[NR, NC], [NR, NC], [NR, NC], [33, 257], [0, 5], [NR, NC]], dtype=np.int32)
    C = torch.from_numpy(V).cuda()
    col, value, wit = solve_wit(C, shapes=shapes)
    col, wit = col.copy(), wit.copy()
    col[0, ::3] = [2 ** 31 - 1, -2 ** 31, NC, -2, 4096, 65536, -65536, 10 ** 9][:len(col[0, ::3])] * 3
    wit[1] = rng.integers(0, 256, size=NR)
    wit[2] = 255
    col[3, 40] = 7          # a padded row with a column
    col[3, 5] = 257         # the first column beyond the live ones
    wit[3, 33:] = 1         # marks on padded rows do not count
    col[4, 1] = 0           # an empty instance whose col is not all -1
    col[5] = -1             # an integer instance presented as infeasible
    got = check(C, col, value, wit, shapes=shapes)
    v = to_host(value)
    for b, (r, c) in enumerate(shapes):
        want = lbap_check_ref(V[b], col[b], v[b], wit[b], shape=(r, c))
        assert tuple(got[b]) == want, (b, got[b], want)
    assert got[0, 2] & 1 and got[2, 2] & 4 and got[3, 2] & 1 and got[4, 2] == 1 and got[5, 2] & 9 == 9
    assert got[3, 0] == int((wit[3, :33] != 0).sum())


def test_front_end_returns_the_witness_over_the_shorter_side():
    rng = np.random.default_rng(35)
    for nr, nc in ((30, 45), (45, 30)):
        C = rng.integers(-5, 6, size=(nr, nc)).astype(np.float64)
        for maximize in (False, True):
            r, c, v, w = linear_bottleneck_assignment(C, maximize=maximize, witness=True)
            r0, c0, v0 = linear_bottleneck_assignment(C, maximize=maximize)
            assert np.array_equal(r, r0) and np.array_equal(c, c0) and v == v0
            W = C if nr <= nc else C.T
            _, rval, rwit = lbap_witness_ref(W, maximize)
            assert w.dtype == bool and w.shape == (min(nr, nc),) and np.array_equal(w, rwit.astype(bool)) and v == rval
            col = np.full(W.shape[0], -1)
            col[r if nr <= nc else c] = c if nr <= nc else r
            assert lbap_check_ref(W, col, v, w, maximize)[2] == 0
    r, c, v, w = linear_bottleneck_assignment(np.zeros((0, 4)), witness=True)
    assert r.size == c.size == w.size == 0 and w.dtype == bool
    with pytest.raises(ValueError, match="infeasible"):
        linear_bottleneck_assignment(np.array([[np.inf, np.inf], [1.0, 2.0]]), witness=True)
