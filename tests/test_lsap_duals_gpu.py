"""GPU tests of the dual variables of the batched LSAP solvers and of the
device-side certificate (santa_hip.solve_batched(duals=True), check_duals,
linear_sum_assignment_duals).

The reference is the CPU replay of scipy's loop in lsap_duals_ref.py: integer
duals must equal it, float duals must equal it bit for bit, whichever kernel
ran.  Integer solves are also certified on the device: check_duals' flags == 0
proves an instance optimal without an oracle, which is how the large-batch
launch configurations are checked on every instance here."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lsap_duals_ref as R  # noqa: E402
import lsap_families as F  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

SH_FLAG_EXACT_ARGMIN = 2
SH_FLAG_F64_MW = 16384
SH_FLAG_F64_SW = 32768
INT_FLAGS = (0, SH_FLAG_EXACT_ARGMIN)
F64_FLAGS = (SH_FLAG_F64_SW, SH_FLAG_F64_MW, 0)
COL, SLACK, TIGHT, SIGN, GAP, NONE, RANGE = 1, 2, 4, 8, 16, 32, 64


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    assert [santa_hip.SH_CERT_COL, santa_hip.SH_CERT_SLACK, santa_hip.SH_CERT_TIGHT, santa_hip.SH_CERT_SIGN,
            santa_hip.SH_CERT_GAP, santa_hip.SH_CERT_NONE, santa_hip.SH_CERT_RANGE] == \
        [COL, SLACK, TIGHT, SIGN, GAP, NONE, RANGE]
    return santa_hip


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    """float64 arrays equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def int_batch(family, nr, nc, B):
    """(C int64 [B, nr, nc], col [B, nr], u [B, nr], v [B, nc]) of the replay."""
    C = np.stack([F.instance(family, "int64", nr, nc, k) for k in range(B)])
    rep = [R.replay_instance(family, "int64", nr, nc, k) for k in range(B)]
    return C, np.stack([r[0] for r in rep]), np.stack([r[1] for r in rep]), np.stack([r[2] for r in rep])


@functools.lru_cache(maxsize=None)
def float_batch(family, dtype, nr, nc, B):
    """(C: float64 numpy or a narrow CPU tensor, its float64 image, col, u, v):
    the replay of the widened matrices; an infeasible instance has col -1 and
    NaN duals."""
    inst = [F.instance(family, dtype, nr, nc, k) for k in range(B)]
    C = torch.stack(inst) if dtype in F.NARROW else np.stack(inst)
    C64 = np.stack([F.as_float64(x) for x in inst])
    cols, us, vs = [], [], []
    for k in range(B):
        try:
            col, u, v = R.replay_instance(family, dtype, nr, nc, k) if dtype == "float64" else R.replay(C64[k])
        except ValueError:
            col, u, v = -np.ones(nr, dtype=np.int64), np.full(nr, np.nan), np.full(nc, np.nan)
        cols.append(col), us.append(u), vs.append(v)
    return C, C64, np.stack(cols), np.stack(us), np.stack(vs)


# --------------------------------------------------------------------------- integer
INT_SHAPES = [(64, 64), (63, 64), (65, 65), (255, 256), (257, 257), (300, 513)]
INT_CASES = [(f, nr, nc, "int64") for f in F.INT_FAMILIES for nr, nc in INT_SHAPES]
INT_CASES += [(f, 1000, 1024, "int64") for f in ("mw", "window_edges")]
INT_CASES += [(f, nr, nc, "int32") for f in F.INT32_FAMILIES for nr, nc in INT_SHAPES]
INT_CASES += [("mw", 1000, 1024, "int32")]


@pytest.mark.parametrize("family,nr,nc,dtype", INT_CASES, ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in INT_CASES])
def test_integer_duals_equal_the_replay_and_certify(sh, family, nr, nc, dtype):
    C, rcol, ru, rv = int_batch(family, nr, nc, 2 if nc == 1024 else 3)
    Ct = torch.from_numpy(C).cuda()
    if dtype == "int32":
        Ct = Ct.to(torch.int32)
        assert torch.equal(Ct.cpu().long(), torch.from_numpy(C))  # (the family fits int32)
    for flags in INT_FLAGS:
        col0, cost0 = sh.solve_batched(Ct, flags=flags)
        col, cost, u, v = sh.solve_batched(Ct, flags=flags, duals=True)
        assert u.dtype == torch.int64 and v.dtype == torch.int64
        assert torch.equal(col, col0) and torch.equal(cost, cost0), (family, nr, nc, dtype, flags)
        assert np.array_equal(col.cpu().numpy(), rcol), (family, nr, nc, dtype, flags)
        assert np.array_equal(u.cpu().numpy(), ru) and np.array_equal(v.cpu().numpy(), rv), (family, nr, nc, flags)
        smin, tmax, gap, fl = sh.check_duals(Ct, col, u, v)
        assert fl.cpu().tolist() == [0] * C.shape[0], (family, nr, nc, dtype, flags, fl.cpu().tolist())
        assert smin.dtype == torch.int64 and bool((smin >= 0).all()) and not tmax.any() and not gap.any()
        # the certificate's minimum is the minimum: numpy's, in exact integers
        want = (C.astype(object) - ru.astype(object)[:, :, None] - rv.astype(object)[:, None, :]).min(axis=(1, 2)) \
            if nc <= 65 else None
        if want is not None:
            assert smin.cpu().tolist() == [int(x) for x in want]


# --------------------------------------------------------------------------- float
F64_SHAPES = [(1, 65), (64, 65), (100, 257), (300, 513), (600, 1024)]
F64_CASES = [(f, nr, nc, "float64") for f in F.F64_FAMILIES for nr, nc in F64_SHAPES]
F64_CASES += [(f, nr, nc, d) for d in sorted(F.NARROW) for f in F.NARROW_NAMES for nr, nc in ((100, 257), (300, 513))]


@pytest.mark.parametrize("family,nr,nc,dtype", F64_CASES, ids=[f"{f}-{nr}x{nc}-{d}" for f, nr, nc, d in F64_CASES])
def test_float_duals_are_the_replays_bits(sh, family, nr, nc, dtype):
    """One wave, four waves and the default choice return the same bits, those
    of the replay of the widened matrix; check_duals' minimum slack and largest
    matched slack are numpy's for the same duals, bit for bit."""
    C, C64, rcol, ru, rv = float_batch(family, dtype, nr, nc, 1 if nc == 1024 else 2)
    Cd = C.cuda() if dtype in F.NARROW else torch.from_numpy(C).cuda()
    B = C64.shape[0]
    feasible = (rcol >= 0).all(axis=1)
    got = []
    for flags in F64_FLAGS:
        col0, cost0 = sh.solve_batched(Cd, flags=flags)
        col, cost, u, v = sh.solve_batched(Cd, flags=flags, duals=True)
        assert u.dtype == torch.float64 and v.dtype == torch.float64
        assert torch.equal(col, col0) and torch.equal(bits(cost), bits(cost0)), (family, nr, nc, dtype, flags)
        assert np.array_equal(col.cpu().numpy(), rcol), (family, nr, nc, dtype, flags)
        assert same_bits(u.cpu().numpy(), ru) and same_bits(v.cpu().numpy(), rv), (family, nr, nc, dtype, flags)
        got.append((u, v))
    for u, v in got[1:]:
        assert torch.equal(bits(u), bits(got[0][0])) and torch.equal(bits(v), bits(got[0][1]))
    u, v = got[0]
    smin, tmax, gap, fl = sh.check_duals(Cd, col, u, v)
    assert smin.dtype == torch.float64 and fl.dtype == torch.int32
    smin, tmax, fl = smin.cpu().numpy(), tmax.cpu().numpy(), fl.cpu().numpy()
    un, vn = u.cpu().numpy(), v.cpu().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            if not feasible[b]:
                assert fl[b] == NONE
                continue
            assert not fl[b] & (COL | NONE | GAP | RANGE), (family, nr, nc, dtype, b, fl[b])
            S = (C64[b] - un[b][:, None]) - vn[b][None, :]
            assert same_bits(smin[b], S.min()), (family, nr, nc, dtype, b, smin[b], S.min())
            assert same_bits(tmax[b], np.abs(S[np.arange(nr), rcol[b]]).max()), (family, nr, nc, dtype, b)


def test_infeasible_float_instance_gets_nan_duals_and_none(sh):
    rng = np.random.default_rng(77)
    C = rng.random((3, 40, 100))
    C[1, 5, :] = np.inf  # a row without a finite entry
    Cd = torch.from_numpy(C).cuda()
    for flags in F64_FLAGS:
        col, cost, u, v = sh.solve_batched(Cd, flags=flags, duals=True)
        assert bool((col[1] == -1).all()) and float(cost[1]) == 0.0
        assert bool(torch.isnan(u[1]).all()) and bool(torch.isnan(v[1]).all())
        for b in (0, 2):
            rc, ru, rv = R.replay(C[b])
            assert np.array_equal(col[b].cpu().numpy(), rc)
            assert same_bits(u[b].cpu().numpy(), ru) and same_bits(v[b].cpu().numpy(), rv)
        fl = sh.check_duals(Cd, col, u, v)[3].cpu().tolist()
        assert fl[1] == NONE and not (fl[0] | fl[2]) & (NONE | COL)


# --------------------------------------------------------------------------- surface
@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_ragged_batch_has_zero_padding_in_the_duals(sh, dtype):
    NR, NC = 40, 70
    shapes = [(0, 0), (1, 1), (5, 9), (NR, NC)]
    rng = np.random.default_rng(5)
    if dtype == "int64":
        C = np.full((4, NR, NC), -(1 << 49), dtype=np.int64)  # (padding that would win every argmin)
        live = [rng.integers(-50, 50, size=s, dtype=np.int64) for s in shapes]
    else:
        C = np.full((4, NR, NC), np.nan)
        live = [rng.random(s) for s in shapes]
    for b, (nr, nc) in enumerate(shapes):
        C[b, :nr, :nc] = live[b]
    Cd = torch.from_numpy(C).cuda()
    col0, cost0 = sh.solve_batched(Cd, shapes=shapes)
    col, cost, u, v = sh.solve_batched(Cd, shapes=shapes, duals=True)
    assert torch.equal(col, col0) and torch.equal(bits(cost), bits(cost0))
    un, vn = u.cpu().numpy(), v.cpu().numpy()
    for b, (nr, nc) in enumerate(shapes):
        assert not un[b, nr:].any() and not vn[b, nc:].any(), b
        assert not np.isnan(un[b]).any() and not np.isnan(vn[b]).any()
        if nr:
            rc, ru, rv = R.replay(live[b])
            assert np.array_equal(col[b, :nr].cpu().numpy(), rc)
            assert same_bits(un[b, :nr].astype(np.float64), ru.astype(np.float64))
            assert same_bits(vn[b, :nc].astype(np.float64), rv.astype(np.float64))
    smin, tmax, gap, fl = sh.check_duals(Cd, col, u, v, shapes=shapes)
    if dtype == "int64":
        assert fl.cpu().tolist() == [0, 0, 0, 0]
    else:
        assert not any(f & (COL | NONE | SIGN) for f in fl.cpu().tolist())
    assert not np.isnan(smin.cpu().numpy().astype(np.float64)).any()
    # a padded row that claims a column is no assignment
    bad = col.clone()
    bad[2, 7] = 3
    assert sh.check_duals(Cd, bad, u, v, shapes=shapes)[3].cpu().tolist()[2] & COL


@pytest.mark.parametrize("nr,nc", [(65, 64), (300, 100)])
def test_tall_batch_swaps_the_roles(sh, nr, nc):
    rng = np.random.default_rng(nr)
    C = rng.integers(-1000, 1000, size=(2, nr, nc), dtype=np.int64)
    Cd = torch.from_numpy(C).cuda()
    col0, cost0 = sh.solve_batched(Cd)
    col, cost, u, v = sh.solve_batched(Cd, duals=True)
    assert torch.equal(col, col0) and torch.equal(cost, cost0)
    assert tuple(u.shape) == (2, nr) and tuple(v.shape) == (2, nc)
    assert bool((u <= 0).all()) and bool((u[col < 0] == 0).all()) and int((col < 0).sum()) == 2 * (nr - nc)
    for b in range(2):  # the transposed solve's duals
        rc, ru, rv = R.replay(C[b].T)
        assert np.array_equal(u[b].cpu().numpy(), rv) and np.array_equal(v[b].cpu().numpy(), ru)
    assert bool((Cd - u[:, :, None] - v[:, None, :] >= 0).all())
    smin, tmax, gap, fl = sh.check_duals(Cd, col, u, v)
    assert fl.cpu().tolist() == [0, 0] and bool((smin >= 0).all())
    dup = col.clone()
    i, k = [int(x) for x in torch.nonzero(col[1] >= 0)[:2, 0]]
    dup[1, i] = dup[1, k]  # two rows on one column: found before the inversion
    fl = sh.check_duals(Cd, dup, u, v)[3].cpu().tolist()
    assert fl[0] == 0 and fl[1] & COL


@pytest.mark.parametrize("nr,nc", [(50, 80), (80, 50)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_maximize_returns_dominating_duals(sh, nr, nc, dtype):
    C = torch.from_numpy(np.random.default_rng(3).integers(-500, 500, size=(2, nr, nc))).to(dtype).cuda()
    col0, cost0 = sh.solve_batched(C, maximize=True)
    col, cost, u, v = sh.solve_batched(C, maximize=True, duals=True)
    assert torch.equal(col, col0) and torch.equal(cost, cost0)
    S = u[:, :, None] + v[:, None, :] - C.long()
    assert bool((S >= 0).all())
    live = col >= 0
    assert not S.gather(2, col.clamp(min=0).long()[:, :, None])[:, :, 0][live].any()
    assert int(u.sum() + v.sum()) == int(cost.sum())
    fl = sh.check_duals(C, col, u, v, maximize=True)[3]
    assert fl.cpu().tolist() == [0, 0]
    assert any(sh.check_duals(C, col, u, v)[3].cpu().tolist())  # (not a certificate of the minimum)


def test_linear_sum_assignment_duals_front_end(sh):
    rng = np.random.default_rng(11)
    for C, maximize in ((rng.integers(0, 100, size=(30, 50)), False), (rng.integers(0, 100, size=(50, 30)), False),
                        (rng.integers(0, 100, size=(50, 30)), True), (rng.random((40, 60)), False),
                        (rng.integers(0, 100, size=(20, 20)).astype(np.int64) << 48, False)):
        r, c, u, v = sh.linear_sum_assignment_duals(C, maximize=maximize)
        r0, c0 = sh.linear_sum_assignment(C, maximize=maximize)
        wr, wc = oracle.lsap(-C if maximize else C)
        assert np.array_equal(r, wr) and np.array_equal(c, wc) and np.array_equal(r, r0) and np.array_equal(c, c0)
        try:
            from scipy.optimize import linear_sum_assignment as lsa
            sr, sc = lsa(C, maximize=maximize)
            assert np.array_equal(r, sr) and np.array_equal(c, sc)
        except ImportError:
            pass
        assert u.shape == (C.shape[0],) and v.shape == (C.shape[1],)
        exact = np.issubdtype(C.dtype, np.integer) and int(np.abs(C).max()) < (1 << 40)
        assert u.dtype == v.dtype == (np.int64 if exact else np.float64)
        if exact:
            S = C - u[:, None] - v[None, :]
            assert (S <= 0).all() if maximize else (S >= 0).all()
            assert not S[r, c].any() and int(u.sum() + v.sum()) == int(C[r, c].sum())
    z = sh.linear_sum_assignment_duals(np.zeros((0, 4)))
    assert [a.size for a in z] == [0, 0, 0, 4]


# --------------------------------------------------------------------------- large batches, certified on the device
@pytest.mark.parametrize("B,nr,nc", [(4096, 100, 128), (65536, 8, 200)], ids=["1x2-4096x100x128", "1x4-65536x8x200"])
def test_large_batch_configs_are_certified_on_every_instance(sh, B, nr, nc):
    """One wave per instance with 2 (B >= 4096, nc <= 128) and 4 (B >= 65536,
    nc <= 256) columns per thread: flags == 0 proves each of the B solves
    optimal; 64 of them are also compared with the replay."""
    g = torch.Generator(device="cuda").manual_seed(4200 + nc)
    C = torch.randint(0, 1 << 16, (B, nr, nc), generator=g, dtype=torch.int32, device="cuda")
    col0, cost0 = sh.solve_batched(C)
    col, cost, u, v = sh.solve_batched(C, duals=True)
    assert torch.equal(col, col0) and torch.equal(cost, cost0)
    smin, tmax, gap, fl = sh.check_duals(C, col, u, v)
    assert int(torch.count_nonzero(fl)) == 0
    assert bool((smin >= 0).all()) and not tmax.any() and not gap.any()
    idx = torch.arange(64, device="cuda") * (B // 64) + 17
    Ch, ch, uh, vh = C[idx].cpu().numpy(), col[idx].cpu().numpy(), u[idx].cpu().numpy(), v[idx].cpu().numpy()
    for k in range(64):
        rc, ru, rv = R.replay(Ch[k])
        assert np.array_equal(ch[k], rc) and np.array_equal(uh[k], ru) and np.array_equal(vh[k], rv), (B, k)


# --------------------------------------------------------------------------- the certificate refuses what is wrong
@functools.lru_cache(maxsize=None)
def unique_optimum_batch():
    """Four 20 x 30 instances of i * nc + j plus noise, each with a unique
    optimum: forbidding any chosen entry makes the best assignment dearer."""
    nr, nc, out = 20, 30, []
    rng = np.random.default_rng(2024)
    i, j = np.indices((nr, nc))
    while len(out) < 4:
        C = (i * nc + j + rng.integers(0, 5000, size=(nr, nc))).astype(np.int64)
        _, col = oracle.lsap(C)
        best = int(C[np.arange(nr), col].sum())
        unique = True
        for r in range(nr):
            D = C.copy()
            D[r, col[r]] = 1 << 40
            _, c2 = oracle.lsap(D)
            unique &= int(D[np.arange(nr), c2].sum()) > best
        if unique:
            out.append(C)
    return np.stack(out)


def test_certificate_names_each_corruption(sh):
    C = unique_optimum_batch()
    Cd = torch.from_numpy(C).cuda()
    col, cost, u, v = sh.solve_batched(Cd, duals=True)
    assert sh.check_duals(Cd, col, u, v)[3].cpu().tolist() == [0, 0, 0, 0]

    def flags_of(b, col=col, u=u, v=v):
        fl = sh.check_duals(Cd, col, u, v)[3].cpu().tolist()
        assert all(f == 0 for k, f in enumerate(fl) if k != b), fl
        return fl[b]

    x = u.clone()
    x[1, 7] += 1  # row 7's chosen entry now has slack -1
    assert flags_of(1, u=x) == SLACK | TIGHT | GAP
    x = u.clone()
    x[2, 0] -= 1  # feasible, no longer tight
    assert flags_of(2, u=x) == TIGHT | GAP
    x = col.clone()
    x[3, 4], x[3, 9] = col[3, 9], col[3, 4]  # another assignment: dearer, the optimum being unique
    f = flags_of(3, col=x)
    assert f & TIGHT and not f & (COL | SLACK | SIGN | NONE | RANGE)
    x = col.clone()
    x[0, 5] = col[0, 6]
    assert flags_of(0, col=x) & COL
    x = col.clone()
    x[0, 5] = 30  # outside [0, nc)
    assert flags_of(0, col=x) & COL
    free = sorted(set(range(30)) - set(col[1].cpu().tolist()))[0]
    x = v.clone()
    x[1, free] = 1
    assert flags_of(1, v=x) & SIGN
    x = v.clone()
    x[1, free] = -1  # a free column must stay at 0
    assert flags_of(1, v=x) & SIGN
    x = u.clone()
    x[2, 3] = 1 << 61
    assert flags_of(2, u=x) & RANGE
