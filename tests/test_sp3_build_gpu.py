"""santa_sp3_kernel's fused tile build: one walk of the
wishlist per row in groups of 16 wishes, and the second walk of the rows with
more than 32 entries after the last batch.

Crafted blocks at the smallest shapes where the build can go wrong.  Every
case first asserts on the CPU, from `wish` and `types` alone, the property it
is named for (its rows' entry counts); then the sparse kernel
(SH_FLAG_SP_TILE) must equal the oracle's round -- col, exact cost, per-block
steps, the new type vector and the happiness deltas -- and, with
SH_FLAG_BUILD_ONLY, return the identity assignment at the oracle's cost of it
(the build's own codes)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NG, NQ = 400, 75   # small data: 30000 children; a crafted block holds types below FILL0 only
FILL0 = 256        # first gift type no crafted block holds
OVF_CAP = 384      # overflow entries a block of the fused design holds (SP4_OVF_CAP)


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


@pytest.fixture(scope="module")
def datas(sh):
    """Small data per wishlist length (made once, never changed)."""
    from santa_hip import data as D
    return {nw: D.synthetic(seed=5, nc=NG * NQ, ng=NG, nq=NQ, n_wish=nw, n_good=50) for nw in (4, 16, 20, 100)}


def craft(sd, blocks):
    """Block q = the q-th last run of n children; child j of it holds
    col_types[j] and wishes[j] = {position: gift type}, every other position
    a type no block holds.  -> wish, types, rows [B, n]."""
    nw = sd.n_wish
    n = len(blocks[0][0])
    wish, types = sd.wish.copy(), sd.types.copy()
    rows = np.empty((len(blocks), n), dtype=np.int32)
    for q, (col_types, wishes) in enumerate(blocks):
        assert len(col_types) == n and len(wishes) == n and max(col_types) < FILL0
        kids = np.arange(sd.nc - (q + 1) * n, sd.nc - q * n, dtype=np.int32)
        rows[q] = kids
        types[kids] = np.asarray(col_types, dtype=np.int16)
        for j, w in enumerate(wishes):
            assert all(0 <= p < nw for p in w)
            line = np.arange(FILL0, FILL0 + nw, dtype=np.int16)
            for p, g in w.items():
                line[p] = g
            wish[kids[j]] = line
    return wish, types, rows


def entries(wish, types, rows_b):
    """Tile entries per row of one block: the columns holding each wished type."""
    cnt = np.bincount(types[rows_b], minlength=NG)
    return cnt[wish[rows_b]].sum(axis=1)


def at_random(rng, nw, gifts):
    """{position: gift} with the gifts in this order at increasing random positions."""
    pos = np.sort(rng.choice(nw, len(gifts), replace=False))
    return {int(p): int(g) for p, g in zip(pos, gifts)}


def check(sh, sd, wish, types0, rows, expect_fallback=None, budget=0):
    """The kernel's round on `rows` against the oracle's, then the build alone."""
    from santa_hip import _lib, data as D
    B, n = rows.shape
    t_host = types0.copy()
    osteps = np.zeros(B, dtype=np.int64)
    ocol = np.zeros((B, n), dtype=np.int64)
    ocost = np.zeros(B, dtype=np.int64)
    for b in range(B):
        st = np.zeros(2, dtype=np.uint64)
        ocol[b], ocost[b] = (x[0] for x in oracle.round_blocks(0, wish, t_host, rows[b:b + 1], stats=st, ng=NG))
        osteps[b] = int(st[0])
    s0 = oracle.score_sums(wish, sd.goodkids, types0)
    s1 = oracle.score_sums(wish, sd.goodkids, t_host)
    ident = np.array([np.trace(oracle.cost_single(wish, types0, rows[b], ng=NG)) for b in range(B)], dtype=np.int64)
    c = sh.SantaGPU.from_data(D.SantaData(wish, sd.goodkids, sd.types, sd.nq), 0)
    try:
        c.set_sparse_budget(budget)
        r = torch.from_numpy(np.ascontiguousarray(rows.reshape(-1), dtype=np.int32)).cuda()
        for build_only in (False, True):
            types = c.upload_types(types0)
            col = torch.full((B * n,), -1, dtype=torch.int32, device="cuda")
            cost = torch.zeros(B, dtype=torch.int64, device="cuda")
            delta = torch.zeros(2, dtype=torch.int64, device="cuda")
            steps = torch.zeros(B, dtype=torch.int64, device="cuda")
            c.solve_blocks(0, r, n, types, col=col, cost=cost, delta=delta, steps=steps,
                           flags=_lib.SH_FLAG_SP_TILE | (_lib.SH_FLAG_BUILD_ONLY if build_only else 0))
            gcol = col.cpu().numpy().reshape(B, n)
            if build_only:
                assert np.array_equal(gcol, np.broadcast_to(np.arange(n), (B, n)))
                assert np.array_equal(cost.cpu().numpy(), ident)
                assert np.array_equal(types.cpu().numpy(), types0)
            else:
                assert np.array_equal(gcol, ocol)
                assert np.array_equal(cost.cpu().numpy(), ocost)
                assert np.array_equal(steps.cpu().numpy(), osteps)
                assert np.array_equal(types.cpu().numpy(), t_host)
                assert delta.cpu().tolist() == [s1[0] - s0[0], s1[1] - s0[1]]
            assert c.error_flags() == 0
            if expect_fallback is not None:
                assert c.fallback_blocks() == expect_fallback
    finally:
        c.set_sparse_budget(0)
        c.close()


# --------------------------------------------------------------------------- batch and group edges
@pytest.mark.parametrize("nw", [4, 16, 20, 100])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 255, 256])
def test_sizes(sh, datas, n, nw):
    """Batch boundaries and the half-filled last batch, at fewer wishes than
    one group (4), exactly one group (16), a group and a 4-wish tail (20) and
    the bench's six groups and a tail (100).  Columns hold distinct types but
    for a few pairs; every row wishes up to eight of them at random positions
    (0 and n_wish - 1 among them), two blocks."""
    sd = datas[nw]
    rng = np.random.default_rng([n, nw])
    blocks = []
    for q in range(2):
        ct = rng.permutation(n)
        if n >= 8:  # (rows 0 and n - 1 keep their types: row 0 wishes both)
            ct[1 + rng.choice(n - 2, 3, replace=False)] = ct[1 + rng.choice(n - 2, 3, replace=False)]
        wishes = []
        for j in range(n):
            k = int(rng.integers(0, min(nw, 8, n) + 1))
            w = at_random(rng, nw, rng.choice(np.unique(ct), min(k, len(np.unique(ct))), replace=False))
            wishes.append(w)
        wishes[0] = {0: int(ct[0]), nw - 1: int(ct[n - 1])} if n > 1 else {nw - 1: int(ct[0])}
        blocks.append((ct, wishes))
    wish, types, rows = craft(sd, blocks)
    e = np.concatenate([entries(wish, types, rows[q]) for q in range(2)])
    assert e.max() <= 32 and (n == 1 or e.max() >= 2)  # (no overflow here: that is test_entry_counts)
    check(sh, sd, wish, types, rows, expect_fallback=0)


@pytest.mark.parametrize("nw", [20, 100])
def test_group_boundary_and_last_wish(sh, datas, nw):
    """Rows whose only hits are wishes 15 and 16 (the last of group 0 and the
    first of group 1), rows whose only hit is the last wish, and rows whose
    only hit is the first, in every batch."""
    sd = datas[nw]
    n = 256
    ct = np.random.default_rng(nw).permutation(n)
    wishes = [{3: int(ct[j])} for j in range(n)]
    across, last, first = [0, 63, 64, 130, 255], [1, 62, 65, 191, 254], [2, 66, 192]
    for j in across:
        wishes[j] = {15: int(ct[(j + 1) % n]), 16: int(ct[j])}
    for j in last:
        wishes[j] = {nw - 1: int(ct[j])}
    for j in first:
        wishes[j] = {0: int(ct[j])}
    wish, types, rows = craft(sd, [(ct, wishes)])
    e = entries(wish, types, rows[0])
    assert (e[across] == 2).all() and (e[last] == 1).all() and (e[first] == 1).all()
    for j in across:
        assert (np.flatnonzero(wish[rows[0, j]] < FILL0) == [15, 16]).all()
    for j in last:
        assert (np.flatnonzero(wish[rows[0, j]] < FILL0) == [nw - 1]).all()
    check(sh, sd, wish, types, rows, expect_fallback=0)


# --------------------------------------------------------------------------- entry counts around 32
def count_blocks(rng, n=256):
    """Block A: rows with exactly 31, 32, 33 and 40 entries (rows 5, 70, 6,
    200).  Block B: rows 0, 63, 64 and 255 overflow together (33, 40, 35, 50
    entries).  Block C: twelve rows of 36.  Distinct column types; every
    other row wants its own column's type alone."""
    out = []
    for spec in ({5: 31, 70: 32, 6: 33, 200: 40}, {0: 33, 63: 40, 64: 35, 255: 50},
                 {j: 36 for j in (1, 2, 3, 60, 61, 100, 101, 127, 128, 129, 250, 251)}):
        ct = rng.permutation(n)
        wishes = [{int(rng.integers(0, 100)): int(ct[j])} for j in range(n)]
        for j, k in spec.items():
            wishes[j] = at_random(rng, 100, rng.choice(ct, k, replace=False))
        out.append((ct, wishes, spec))
    return out


def test_entry_counts(sh, datas):
    """Rows below the limit (31), at it without overflow (32), the first
    overflow (33) and a longer list (40); rows 0, 63, 64 and 255 overflowing
    together (the list's allocation across batches)."""
    sd = datas[100]
    blocks = count_blocks(np.random.default_rng(32))
    wish, types, rows = craft(sd, [(ct, w) for ct, w, _ in blocks])
    for q, (_, _, spec) in enumerate(blocks):
        e = entries(wish, types, rows[q])
        assert {j: int(e[j]) for j in spec} == spec
        assert (np.delete(e, list(spec)) == 1).all()
        assert int((e[e > 32] - 31).sum()) <= OVF_CAP
    check(sh, sd, wish, types, rows, expect_fallback=0)


@pytest.mark.parametrize("cap,fallback", [(384, 0), (60, 0), (59, 1), (34, 1), (33, 2), (11, 2), (10, 3)])
def test_overflow_budget(sh, datas, cap, fallback):
    """The overflow list at a budget that sends some blocks to the fallback
    launch: the three blocks of test_entry_counts need 11, 34 and 60 entries."""
    sd = datas[100]
    blocks = count_blocks(np.random.default_rng(32))
    wish, types, rows = craft(sd, [(ct, w) for ct, w, _ in blocks])
    need = []
    for q in range(3):
        e = entries(wish, types, rows[q])
        need.append(int((e[e > 32] - 31).sum()))
    assert need == [11, 34, 60]
    assert sum(x > cap for x in need) == fallback
    check(sh, sd, wish, types, rows, expect_fallback=fallback, budget=16 * cap)


# --------------------------------------------------------------------------- types on several columns
def test_multi_column_types(sh, datas):
    """Types on 2, 3, 4 and 9 columns of the block (the head word's third
    column, the csort list), as a row's first, middle and last hit, and
    straddling entry 31: 30 + 2 (ends at the limit), 31 + 2, 30 + 3, 29 + 4,
    29 + 9 and 25 + 9 (slots 25..33)."""
    sd = datas[100]
    n = 256
    rng = np.random.default_rng(9)
    ct = np.arange(n)
    cols = rng.permutation(n)
    multi = {2: 0, 3: 1, 4: 2, 9: 3}  # columns -> type
    pos = 0
    for k, t in multi.items():
        ct[cols[pos:pos + k]] = t
        pos += k
    ct[cols[pos:]] = np.arange(4, 4 + n - pos)
    singles = np.arange(4, 4 + n - pos)
    wishes = [{int(rng.integers(0, 100)): int(ct[j])} for j in range(n)]
    want = {}
    row = iter(rng.permutation(n))
    for k, t in multi.items():  # first, middle, last hit of a short row
        for where in range(3):
            g = list(rng.choice(singles, 2, replace=False))
            g.insert(where, t)
            j = int(next(row))
            wishes[j] = at_random(rng, 100, g)
            want[j] = 2 + k
    for before, k in ((30, 2), (31, 2), (30, 3), (29, 4), (29, 9), (25, 9)):
        for after in (0, 2):
            g = list(rng.choice(singles, before + after, replace=False))
            g.insert(before, multi[k])
            j = int(next(row))
            wishes[j] = at_random(rng, 100, g)
            want[j] = before + k + after
    wish, types, rows = craft(sd, [(ct, wishes)])
    cnt = np.bincount(types[rows[0]], minlength=NG)
    assert [int(cnt[t]) for t in multi.values()] == list(multi)
    e = entries(wish, types, rows[0])
    assert {j: int(e[j]) for j in want} == want
    assert 32 in want.values() and 33 in want.values() and int((e[e > 32] - 31).sum()) <= OVF_CAP
    check(sh, sd, wish, types, rows, expect_fallback=0)


def test_type_on_255_columns_declines(sh, datas):
    """A type on 255 columns: the block is left to the fallback launch."""
    sd = datas[100]
    n = 256
    ct = np.full(n, 7)
    ct[100] = 8
    wishes = [{} for _ in range(n)]
    for j in (0, 63, 100, 255):
        wishes[j] = {5: 8, 40: 7}
    wish, types, rows = craft(sd, [(ct, wishes)])
    assert np.bincount(types[rows[0]], minlength=NG)[7] == 255
    assert (entries(wish, types, rows[0])[[0, 63, 100, 255]] == 256).all()
    check(sh, sd, wish, types, rows, expect_fallback=1)


# --------------------------------------------------------------------------- the own code
@pytest.mark.parametrize("nw", [4, 16, 20, 100])
def test_own_type_positions(sh, datas, nw):
    """A child that wishes the type it holds: as its first wish, as its last,
    at the last wish of a group and the first of the next; in the first, a
    middle and the half-filled last batch.  (A wishlist holds a gift once:
    the context refuses a repeated one.)"""
    sd = datas[nw]
    n = 130
    ct = np.random.default_rng(nw + 1).permutation(n)
    wishes = [{1: int(ct[(j + 1) % n])} for j in range(n)]
    own_at = {0: [0], 63: [nw - 1], 64: [0], 129: [nw - 1], 128: [0], 65: [min(15, nw - 1)], 66: [min(16, nw - 1)]}
    for j, ps in own_at.items():
        for p in ps:
            wishes[j][p] = int(ct[j])
    wish, types, rows = craft(sd, [(ct, wishes)])
    for j, ps in own_at.items():
        assert (np.flatnonzero(wish[rows[0, j]] == types[rows[0, j]]) == sorted(set(ps))).all()
    check(sh, sd, wish, types, rows, expect_fallback=0)
