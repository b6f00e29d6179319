"""The min-sum certificate (check_duals, check_duals_large: lsap_cert_kernel,
lsap_slack_kernel, lsap_cert_final_kernel) against its host reference
(lsap_cert_ref.cert_ref), entry by entry.

The instances are certified by construction (lsap_cert_families.py) and a plant
lowers ONE entry below u[i] + v[j]: the only negative slack of its instance, so
a pass over the corner that loses that entry returns 0 where the reference
returns -d.  The plants walk the edges of the launch geometry (the last row of
a chunk, the last register stripe, the tail of a partial pack, the last
workgroup) in every instance of every case, and in the exhaustive cases every
entry of the corner is planted in exactly one instance.  smin, tmax, gap and
flags must equal the reference's: integers exactly, floats bit for bit (any NaN
matching any NaN).  test_lsap_cert_cpu.py proves the reference, the plants and
that the cases reach every class of launch."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_cert_families as CF  # noqa: E402
from lsap_cert_ref import COL, GAP, RANGE, SLACK, TIGHT, cert_ref, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


def tt(a):
    """A torch tensor holding a copy of a (read-only) numpy array."""
    return torch.from_numpy(np.array(a))


def to_torch(S, dt):
    return tt(np.asarray(S).view(np.int16)).view(torch.bfloat16) if dt == "bf16" else tt(S)


def unaligned(C):
    """A contiguous copy of C that starts one element into its buffer."""
    buf = torch.empty(C.numel() + 1, dtype=C.dtype, device=C.device)
    out = buf[1:].view(C.shape)
    out.copy_(C)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def fresh(C0, aligned=True):
    C = C0.clone() if aligned else unaligned(C0)
    assert aligned == (C.data_ptr() % 16 == 0)
    return C


def run(sh, C, col, u, v, shapes=None, large=False, maximize=False):
    """-> (smin, tmax, gap, flags) as numpy arrays [B]."""
    out = (sh.check_duals_large if large else sh.check_duals)(C, col, u, v, shapes=shapes, maximize=maximize)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def agrees(got, b, want, dt):
    smin, tmax, gap, flags = (x[b] for x in got)
    if dt in CF.FLOATS:
        return bool(same_bits(smin, want[0]) and same_bits(tmax, want[1]) and same_bits(gap, want[2])
                    and int(flags) == want[3])
    if want[3] & RANGE:     # the other bits and the values are unspecified
        return bool(flags & RANGE)
    return (int(smin), int(tmax), int(gap), int(flags)) == want


def ref_dtype(W, dt):
    return W.astype(np.int32) if dt == "i32" else W


def plant_tensor(vals, dt, dev):
    """The plants' widened values in the cost dtype (exact: plant_value has checked each)."""
    if dt in CF.FLOATS:
        return torch.tensor(vals, dtype=torch.float64).to({"f64": torch.float64, "f32": torch.float32,
                                                           "f16": torch.float16, "bf16": torch.bfloat16}[dt]).to(dev)
    return torch.tensor(vals, dtype=torch.int64).to(torch.int32 if dt == "i32" else torch.int64).to(dev)


@functools.lru_cache(maxsize=None)
def host_batch(case):
    return CF.batch(case)


@functools.lru_cache(maxsize=None)
def expected(case, b, pos):
    """cert_ref of member b of the case's batch (padding and all) with the
    plant at pos, or pristine for pos None.  Members of a batch of one shape
    repeat with period SEEDS: computed once."""
    S, col, u, v = host_batch(case)
    W = CF.widen(S[b], case.dt).copy()
    if pos is not None:
        W[pos] = CF.plant_value(CF.member(case, b), *pos)
    return cert_ref(ref_dtype(W, case.dt), col[b], u[b], v[b], CF.member_shape(case, b))


def expect(case, b, pos):
    return expected(case, b if case.shapes is not None else b % CF.SEEDS, pos)


def device_batch(case):
    S, col, u, v = host_batch(case)
    shapes = None if case.shapes is None else np.array(case.shapes, dtype=np.int32)
    return (to_torch(S, case.dt).cuda(), tt(col).to(torch.int32).cuda(), tt(u).cuda(),
            tt(v).cuda(), shapes)


# --------------------------------------------------------------------------- B <= 64: every position in every instance
@pytest.mark.parametrize("case", CF.CASES, ids=[CF.case_id(c) + ("-large" if c.large else "") for c in CF.CASES])
def test_every_position_is_seen_in_every_instance(sh, case):
    """Call k plants position P[(k + b) % len(P)] into instance b of a clone of
    the pristine batch: after len(P) calls every instance has had every
    position, and each call differs from instance to instance."""
    C0, col, u, v, shapes = device_batch(case)
    P = [CF.case_positions(case, b) for b in range(case.B)]
    live = [b for b in range(case.B) if P[b]]
    assert live and max(len(p) for p in P) >= 4

    def pristine():
        got = run(sh, fresh(C0, case.aligned), col, u, v, shapes, case.large)
        for b in range(case.B):
            want = expect(case, b, None)
            assert agrees(got, b, want, case.dt), (b, [x[b] for x in got], want)
            assert want[3] == 0 or case.variant == "multiscale"
    pristine()
    for k in range(max(len(p) for p in P)):
        C = fresh(C0, case.aligned)
        pos = [P[b][(k + b) % len(P[b])] for b in live]
        vals = [CF.plant_value(CF.member(case, b), *p) for b, p in zip(live, pos)]
        C[live, [p[0] for p in pos], [p[1] for p in pos]] = plant_tensor(vals, case.dt, C.device)
        got = run(sh, C, col, u, v, shapes, case.large)
        if not case.aligned:   # the bits of the aligned copy
            again = run(sh, C.clone(), col, u, v, shapes, case.large)
            assert all(same_bits(a, g) if a.dtype == np.float64 else np.array_equal(a, g) for a, g in zip(again, got))
        for b in range(case.B):
            p = pos[live.index(b)] if b in live else None
            want = expect(case, b, p)
            assert agrees(got, b, want, case.dt), (k, b, p, [x[b] for x in got], want)
            if p is not None and case.variant == "plain" and CF.member(case, b).col[p[0]] != p[1]:
                assert int(got[0][b]) == -CF.depth(*p) and got[3][b] == SLACK   # (what the reference said, in words)
    pristine()


# --------------------------------------------------------------------------- B >= 2048: every entry, one instance each
@pytest.mark.parametrize("dt,nr,nc,aligned", CF.EXHAUSTIVE, ids=lambda x: str(x))
def test_every_entry_is_the_minimum_of_one_instance(sh, dt, nr, nc, aligned):
    B = nr * nc
    m = CF.certified(dt, nr, nc, 0)
    C = to_torch(m.S, dt).cuda().expand(B, nr, nc).contiguous()
    C = fresh(C, aligned)
    col = tt(m.col).to(torch.int32).cuda().expand(B, nr).contiguous()
    u = tt(m.u).cuda().expand(B, nr).contiguous()
    v = tt(m.v).cuda().expand(B, nc).contiguous()
    got = run(sh, C, col, u, v)
    assert not got[3].any() and not got[0].any() and not got[1].any() and not got[2].any()
    vals = [CF.plant_value(m, *divmod(k, nc)) for k in range(B)]
    b = torch.arange(B, device=C.device)
    C[b, b // nc, b % nc] = plant_tensor(vals, dt, C.device)
    got = run(sh, C, col, u, v)
    W = CF.widen(m.S, dt)
    for k in range(B):
        i, j = divmod(k, nc)
        P = W.copy()
        P[i, j] = vals[k]
        want = cert_ref(ref_dtype(P, dt), m.col, m.u, m.v)
        chosen = m.col[i] == j
        assert want[0] == -CF.depth(i, j) and want[3] == (SLACK if not chosen else
                                                         SLACK | TIGHT | (0 if dt in CF.FLOATS else GAP))
        assert agrees(got, k, want, dt), (k, i, j, [x[k] for x in got], want)


# --------------------------------------------------------------------------- ragged batches: the padding is not read
RAGGED = [c for c in CF.CASES if c.shapes is not None]


@pytest.mark.parametrize("case", RAGGED, ids=[CF.case_id(c) + ("-large" if c.large else "") for c in RAGGED])
def test_entries_outside_a_corner_are_not_seen(sh, case):
    """The padding holds a poison (test_every_position_.. certifies the corners
    over it and sees the plant at (nr_b - 1, nc_b - 1)); here finite entries far
    below every dual sum lie just outside each corner, at (nr_b, j) and (i, nc_b)."""
    C0, col, u, v, shapes = device_batch(case)
    C = C0.clone()
    for b, (nr, nc) in enumerate(case.shapes):
        if nr < case.NR:
            C[b, nr, :] = -128
        if nc < case.NC:
            C[b, :, nc] = -128
    got = run(sh, C, col, u, v, shapes, case.large)
    for b in range(case.B):
        assert agrees(got, b, (0, 0, 0, 0), case.dt), (b, [x[b] for x in got])
        assert expect(case, b, None) == (0, 0, 0, 0)
    # one row and one column further in, the same entries are seen
    b, (nr, nc) = next((b, s) for b, s in enumerate(case.shapes) if 1 < s[0] < case.NR and s[1] < case.NC)
    m = CF.member(case, b)
    C = C0.clone()
    C[b, nr - 1, :nc] = -128
    got = run(sh, C, col, u, v, shapes, case.large)
    W = CF.widen(host_batch(case)[0][b], case.dt).copy()
    W[nr - 1, :nc] = -128
    want = cert_ref(ref_dtype(W, case.dt), m.col, host_batch(case)[2][b], host_batch(case)[3][b], (nr, nc))
    assert want[0] < 0 and want[3] & SLACK and agrees(got, b, want, case.dt), ([x[b] for x in got], want)


# --------------------------------------------------------------------------- documented values
TORCH_FLOAT = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def one(m, B=1):
    """A certified instance as device tensors [B, ..]."""
    return (to_torch(m.S, m.dt).cuda().expand(B, *m.S.shape).contiguous(),
            tt(m.col).to(torch.int32).cuda().expand(B, -1).contiguous(),
            tt(m.u).cuda().expand(B, -1).contiguous(),
            tt(m.v).cuda().expand(B, -1).contiguous())


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_float_gap_is_summed_in_the_documented_order(sh, dt):
    """The bits of (sum u + sum v) - sum C[i][col[i]] on the input whose bits
    test_lsap_cert_cpu.py shows to depend on the order, the four waves' included."""
    W, col, u, v = CF.gap_input()
    C = tt(W).to(TORCH_FLOAT[dt])
    assert np.array_equal(C.double().numpy(), W)
    want = cert_ref(W, col, u, v)
    got = run(sh, C.cuda()[None], tt(col).to(torch.int32).cuda()[None], tt(u).cuda()[None],
              tt(v).cuda()[None])
    assert same_bits(got[2][0], want[2]), (got[2][0].hex(), float(want[2]).hex())
    assert agrees(got, 0, want, dt), ([x[0] for x in got], want)
    # two members with the rows in another order: other elements per thread, other bits, the reference's again
    p = np.random.default_rng(5).permutation(len(u))
    want_p = cert_ref(W[p], col[p], u[p], v)
    assert not same_bits(want_p[2], want[2])
    got = run(sh, torch.stack([C, C[torch.from_numpy(p)]]).cuda(),
              torch.from_numpy(np.stack([col, col[p]])).to(torch.int32).cuda(),
              torch.from_numpy(np.stack([u, u[p]])).cuda(), torch.from_numpy(np.stack([v, v])).cuda())
    assert agrees(got, 0, want, dt) and agrees(got, 1, want_p, dt), ([x.tolist() for x in got], want, want_p)


@pytest.mark.parametrize("dt", ["i64", "i32"])
def test_integer_tmax_and_gap_that_are_not_zero(sh, dt):
    m = CF.certified(dt, 20, 40, 0)
    C, col, u, v = one(m, 2)
    u[1, 7] -= 3
    got = run(sh, C, col, u, v)
    assert agrees(got, 0, (0, 0, 0, 0), dt) and agrees(got, 1, (0, 3, -3, TIGHT | GAP), dt), [x.tolist() for x in got]
    uh = m.u.copy()
    uh[7] -= 3
    assert cert_ref(ref_dtype(CF.widen(m.S, dt), dt), m.col, uh, m.v) == (0, 3, -3, TIGHT | GAP)
    u[0, 3] += 5   # every slack of the row falls by 5: the minimum too
    got = run(sh, C, col, u, v)
    uh = m.u.copy()
    uh[3] += 5
    want = cert_ref(ref_dtype(CF.widen(m.S, dt), dt), m.col, uh, m.v)
    assert want == (-5, 5, 5, SLACK | TIGHT | GAP) and agrees(got, 0, want, dt), [x.tolist() for x in got]


@pytest.mark.parametrize("dt", CF.FLOATS)
def test_float_special_values(sh, dt):
    """-0.0 as the minimum (below the +0.0 of every chosen entry), a NaN cost,
    a -inf cost, +inf costs that are not the minimum: one instance each."""
    m = CF.certified(dt, 20, 40, 0)
    free = np.setdiff1d(np.arange(40), m.col)
    W = np.stack([CF.widen(m.S, dt)] * 5)
    u, v = np.stack([m.u] * 5), np.stack([m.v] * 5)
    i, j = 19, int(free[-1])
    W[0, i, :] -= u[0, i]            # u[i] = 0 and a free column: (-0.0 - 0) - 0 = -0.0
    u[0, i] = 0
    W[0, i, j] = -0.0
    W[1, i, j] = np.nan
    W[2, i, j] = -np.inf
    W[3, :, free[0]] = np.inf
    W[3, 0, j] = np.inf
    W[4, i, m.col[i]] = np.nan       # a chosen entry: tmax and the gap are NaN too
    C = tt(W).to(TORCH_FLOAT[dt])
    assert same_bits(C.double().numpy(), W)
    got = run(sh, C.cuda(), torch.from_numpy(np.stack([m.col] * 5)).to(torch.int32).cuda(), tt(u).cuda(),
              tt(v).cuda())
    for b in range(5):
        want = cert_ref(W[b], m.col, u[b], v[b])
        assert agrees(got, b, want, dt), (b, [x[b] for x in got], want)
    assert np.signbit(got[0][0]) and got[0][0] == 0 and got[3][0] == 0
    assert np.isnan(got[0][1]) and got[3][1] == SLACK and got[1][1] == 0 and got[2][1] == 0
    assert got[0][2] == -np.inf and got[3][2] == SLACK
    assert same_bits(got[0][3], 0.0) and got[3][3] == 0
    assert np.isnan(got[0][4]) and np.isnan(got[1][4]) and np.isnan(got[2][4]) and got[3][4] == SLACK | TIGHT


@pytest.mark.parametrize("B,nr,nc", [(1, 300, 320), (64, 300, 304), (2048, 9, 16)])
def test_one_int64_cost_of_2_to_61_sets_range(sh, B, nr, nc):
    """The slack pass alone meets the entry (it is not a chosen one), in the last
    row and in the last workgroup of each regime of the row split."""
    m = CF.certified("i64", nr, nc, 0)
    C, col, u, v = one(m, B)
    j = max(j for j in range(nc) if m.col[nr - 1] != j)
    C[B - 1, nr - 1, j] = 1 << 61
    got = run(sh, C, col, u, v)
    W = CF.widen(m.S, "i64").copy()
    W[nr - 1, j] = 1 << 61
    assert cert_ref(W, m.col, m.u, m.v)[3] & RANGE
    assert got[3][B - 1] & RANGE and not got[3][:B - 1].any(), got[3]
    C[B - 1, nr - 1, j] = (1 << 61) - 1      # one below: an ordinary, large slack
    got = run(sh, C, col, u, v)
    assert not got[3].any() and not got[0].any()


# --------------------------------------------------------------------------- the front end's other paths
@pytest.mark.parametrize("dt", ["i32", "f64", "bf16"])
def test_tall_batches_under_the_same_plants(sh, dt):
    """A tall batch is checked as its transpose with the duals swapped and col
    inverted: the wide instance's certificate, plants and all."""
    nr, nc, B = 20, 30, 3
    M = [CF.certified(dt, nr, nc, b) for b in range(B)]
    col_t = np.full((B, nc), -1, dtype=np.int64)
    for b, m in enumerate(M):
        col_t[b, m.col] = np.arange(nr)
    C0 = torch.stack([to_torch(m.S, dt) for m in M]).transpose(1, 2).contiguous().cuda()   # [B, nc, nr]: tall
    col = tt(col_t).to(torch.int32).cuda()
    u = torch.from_numpy(np.stack([m.v for m in M])).cuda()
    v = torch.from_numpy(np.stack([m.u for m in M])).cuda()
    assert not run(sh, C0, col, u, v)[3].any()
    P = CF.positions(CF.geometry(B, nr, nc, nc, CF.ITEMSIZE[dt]), nr, nc)
    for k in range(len(P)):
        C = C0.clone()
        pos = [P[(k + b) % len(P)] for b in range(B)]
        vals = [CF.plant_value(m, *p) for m, p in zip(M, pos)]
        C[list(range(B)), [p[1] for p in pos], [p[0] for p in pos]] = plant_tensor(vals, dt, C.device)
        got = run(sh, C, col, u, v)
        for b, (m, p) in enumerate(zip(M, pos)):
            want = cert_ref(ref_dtype(CF.planted(m, *p), dt), m.col, m.u, m.v)
            assert agrees(got, b, want, dt), (k, b, p, [x[b] for x in got], want)


@pytest.mark.parametrize("dt", CF.DTYPES)
def test_maximize_under_the_same_plants(sh, dt):
    """maximize certifies (-C, -u, -v): the negated batch gives the bits of the
    minimisation (int32 costs are negated in int64)."""
    nr, nc, B = 20, 40, 3
    M = [CF.certified(dt, nr, nc, b) for b in range(B)]
    C0 = -torch.stack([to_torch(m.S, dt) for m in M]).cuda()
    col = torch.from_numpy(np.stack([m.col for m in M])).to(torch.int32).cuda()
    u = -torch.from_numpy(np.stack([m.u for m in M])).cuda()
    v = -torch.from_numpy(np.stack([m.v for m in M])).cuda()
    assert not run(sh, C0, col, u, v, maximize=True)[3].any()
    P = CF.positions(CF.geometry(B, nr, nc, nc, 8 if dt == "i32" else CF.ITEMSIZE[dt]), nr, nc)
    for k in range(len(P)):
        C = C0.clone()
        pos = [P[(k + b) % len(P)] for b in range(B)]
        vals = [-CF.plant_value(m, *p) for m, p in zip(M, pos)]
        C[list(range(B)), [p[0] for p in pos], [p[1] for p in pos]] = plant_tensor(vals, dt, C.device)
        got = run(sh, C, col, u, v, maximize=True)
        for b, (m, p) in enumerate(zip(M, pos)):
            want = cert_ref(CF.planted(m, *p), m.col, m.u, m.v)
            assert agrees(got, b, want, dt), (k, b, p, [x[b] for x in got], want)


# --------------------------------------------------------------------------- col outside int32
OUTSIDE = [(1 << 32) + 3, -(1 << 32) - 1, (1 << 31), -(1 << 31) - 1, (1 << 40)]


@pytest.mark.parametrize("large", [False, True], ids=["check_duals", "check_duals_large"])
def test_a_col_outside_int32_is_not_an_assignment(sh, large):
    """An int64 col is narrowed by saturation: 2**32 + c must not become column c."""
    m = CF.certified("i64", 8, 12, 0)
    B = len(OUTSIDE) + 2
    C, col, u, v = one(m, B)
    col = col.long()
    col[1, 2] += 1 << 32                      # the right column after a wrap
    for b, x in enumerate(OUTSIDE):
        col[2 + b, b] = x
    got = run(sh, C, col, u, v, large=large)
    assert got[3][0] == 0 and (got[3][1:] & COL).all(), got[3]
    for bad in (col.double(), col.to(torch.float32), col != 0):
        with pytest.raises(TypeError):
            (sh.check_duals_large if large else sh.check_duals)(C, bad, u, v)
    # tall: col passes through its inversion first
    Ct, ut, vt = C.transpose(1, 2).contiguous(), v, u
    col_t = torch.full((B, 12), -1, dtype=torch.int64, device=C.device)
    col_t[:, tt(m.col).cuda()] = torch.arange(8, device=C.device)
    assert not run(sh, Ct, col_t, ut, vt, large=large)[3].any()
    j = int(m.col[2])
    col_t[1, j] += 1 << 32
    col_t[2, j] = -(1 << 32) - 1
    got = run(sh, Ct, col_t, ut, vt, large=large)
    assert got[3][0] == 0 and got[3][1] & COL and got[3][2] & COL and not got[3][3:].any(), got[3]


def test_check_bottleneck_refuses_a_col_outside_int32(sh):
    rng = np.random.default_rng(41)
    for shape in ((8, 12), (12, 8)):
        C = torch.from_numpy(rng.integers(-50, 50, size=(4,) + shape)).cuda()
        col, value, wit = sh.solve_bottleneck_batched(C, witness=True)
        assert not sh.check_bottleneck(C, col, value, wit)[2].any()
        col = col.long()
        assert not sh.check_bottleneck(C, col, value, wit)[2].any()
        i = int((col[1] >= 0).nonzero()[0])
        col[1, i] += 1 << 32
        col[2, i] = -(1 << 32) - 1
        flags = sh.check_bottleneck(C, col, value, wit)[2].cpu().numpy()
        assert flags[0] == 0 and flags[3] == 0 and flags[1] & sh._lib.SH_LBCERT_COL and flags[2] & sh._lib.SH_LBCERT_COL
        with pytest.raises(TypeError):
            sh.check_bottleneck(C, col.double(), value, wit)
