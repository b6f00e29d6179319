"""santa_sp3_kernel's peeled first Dijkstra step: the
single-step tail, the hand-over to the generic loop and the first step of a
row with more than 32 hits, on crafted blocks and on the bench's states.

Every crafted case first asserts, on the oracle or on lsap_families.sap_trace
alone, the property that makes it meaningful; then the sparse kernel
(SH_FLAG_SP_TILE) must equal the oracle's round: col, exact cost, per-block
steps, the new type vector and the happiness deltas."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from lsap_families import sap_trace  # noqa: E402

pytestmark = pytest.mark.gpu

NW, NG, NQ = 100, 400, 75  # small data: 30000 children, types 256.. never in a crafted block
FILL0 = 256                # first gift type no crafted block holds
OVF_CAP = 384              # overflow entries a block of the fused design holds (SP4_OVF_CAP)


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


@pytest.fixture(scope="module")
def small(sh):
    from santa_hip import data as D
    sd = D.synthetic(seed=5, nc=NG * NQ, ng=NG, nq=NQ, n_wish=NW, n_good=50)
    c = sh.SantaGPU.from_data(sd, 0)
    yield sd, c
    c.close()


@pytest.fixture(scope="module")
def ctx(sh, full_data):
    return sh.SantaGPU.from_data(full_data, 0)


def cost_v(wish, ct):
    """The block's cost matrix in lattice units (a wish -a * 512, a miss 1; a
    later duplicate of a gift in a wishlist overwrites, as the kernel's scatter)."""
    nw = wish.shape[1]
    C = np.ones((wish.shape[0], ct.shape[0]), dtype=np.int64)
    for r in range(nw):
        C[ct[None, :] == wish[:, r][:, None]] = -(nw - r) * 512
    return C


def dijkstra_lengths(C):
    """(steps of each Dijkstra, longest augmenting path in hops) of scipy's solve."""
    _, _, first, longest = sap_trace(C)
    starts = np.flatnonzero(np.asarray(first))
    return np.diff(np.append(starts, len(first))), longest


def crafted(sd, col_types, heads):
    """A block of the last len(col_types) children: child j holds col_types[j]
    and wishes heads[j] (gift types, best first), then types no block holds."""
    n = len(col_types)
    kids = np.arange(sd.nc - n, sd.nc, dtype=np.int32)
    wish, types = sd.wish.copy(), sd.types.copy()
    types[kids] = np.asarray(col_types, dtype=np.int16)
    for j, h in enumerate(heads):
        h = list(h)
        fill = [t for t in range(FILL0, NG) if t not in h][:NW - len(h)]
        wish[kids[j]] = np.asarray(h + fill, dtype=np.int16)
    return wish, types, kids.reshape(1, n)


def check_blocks(c, wish, good, types0, rows, flags, apply=True):
    """The kernel's round on `rows` [B, n] from types0 against the oracle's."""
    from santa_hip import _lib
    B, n = rows.shape
    t_host = types0.copy()
    osteps = np.zeros(B, dtype=np.int64)
    ocol = np.zeros((B, n), dtype=np.int64)
    ocost = np.zeros(B, dtype=np.int64)
    for b in range(B):  # (per block: the oracle's step count is a sum over its blocks)
        st = np.zeros(2, dtype=np.uint64)
        ocol[b], ocost[b] = (x[0] for x in oracle.round_blocks(0, wish, t_host, rows[b:b + 1], stats=st,
                                                               ng=good.shape[0]))
        osteps[b] = int(st[0])
    s0 = oracle.score_sums(wish, good, types0)
    s1 = oracle.score_sums(wish, good, t_host)
    types = c.upload_types(types0)
    r = torch.from_numpy(np.ascontiguousarray(rows.reshape(-1), dtype=np.int32)).cuda()
    col = torch.empty(B * n, dtype=torch.int32, device="cuda")
    cost = torch.empty(B, dtype=torch.int64, device="cuda")
    delta = torch.zeros(2, dtype=torch.int64, device="cuda")
    steps = torch.empty(B, dtype=torch.int64, device="cuda")
    c.solve_blocks(0, r, n, types, col=col, cost=cost, delta=delta, steps=steps,
                   flags=flags | (0 if apply else _lib.SH_FLAG_NO_APPLY))
    assert np.array_equal(col.cpu().numpy().reshape(B, n), ocol), flags
    assert np.array_equal(cost.cpu().numpy(), ocost), flags
    assert np.array_equal(steps.cpu().numpy(), osteps), flags
    assert np.array_equal(types.cpu().numpy(), t_host if apply else types0), flags
    assert delta.cpu().tolist() == [s1[0] - s0[0], s1[1] - s0[1]], flags
    assert c.error_flags() == 0
    return osteps


def small_ctx(sh, sd, wish):
    from santa_hip import data as D
    return sh.SantaGPU.from_data(D.SantaData(wish, sd.goodkids, sd.types, sd.nq), 0)


@pytest.mark.parametrize("n", [256, 1, 2, 3, 5, 63, 64, 65, 255])
def test_all_single_step(sh, small, n):
    """Every child ranks a distinct held gift type first: n Dijkstras of one
    step (the byte and lane edges of the c4r / r4c updates at the small n)."""
    from santa_hip import _lib
    sd, _ = small
    perm = np.random.default_rng(n).permutation(n)
    wish, types, rows = crafted(sd, np.arange(n), [[int(perm[j])] for j in range(n)])
    S, _ = dijkstra_lengths(cost_v(wish[rows[0]], types[rows[0]]))
    assert len(S) == n and (S == 1).all()
    c = small_ctx(sh, sd, wish)
    steps = check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE)
    assert steps.tolist() == [n]
    c.close()


def test_no_early_exit(sh, small):
    """Rows 0..39 take the columns 0..39 in turn, each with the next column
    as its second wish; row 40 wants column 0 only, and its path shifts the
    whole chain (41 hops); from row 42 on every row wants the column of the
    row before it first and its own second, so its first step finds an
    assigned column: the hand-over at every row, in every lane and byte."""
    from santa_hip import _lib
    sd, _ = small
    n, m = 256, 40
    heads = [[j, j + 1] for j in range(m)] + [[0], [m + 1]] + [[k - 1, k] for k in range(m + 2, n)]
    order = np.random.default_rng(3).permutation(n)  # (columns anywhere in the lanes)
    wish, types, rows = crafted(sd, order, [[int(order[t]) for t in h] for h in heads])
    S, longest = dijkstra_lengths(cost_v(wish[rows[0]], types[rows[0]]))
    assert (S > 1).sum() >= n // 2 and longest >= 32
    c = small_ctx(sh, sd, wish)
    check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE)
    c.close()


def test_first_step_ties(sh, small):
    """Ties at the first step.  Rows whose wishes miss every type of the
    block: all columns tie, the last unassigned one in scan order wins.  Rows
    that want a type held by three columns: the second and third of them tie
    between its assigned and unassigned columns and take an unassigned one in
    one step, the fourth finds all three assigned and goes on."""
    from santa_hip import _lib
    sd, _ = small
    n = 256
    col_types = np.arange(n)
    col_types[[7, 130, 201]] = 7          # one type on three columns
    want7 = [3, 7, 64, 65, 127, 200, 255]  # rows that want it (and nothing else the block holds)
    allmiss = [0, 1, 66, 128, 254]
    heads = [[int(col_types[j])] for j in range(n)]
    for j in want7:
        heads[j] = [7]
    for j in allmiss:
        heads[j] = []
    wish, types, rows = crafted(sd, col_types, heads)
    C = cost_v(wish[rows[0]], types[rows[0]])
    assert (C[allmiss] == 1).all()
    S, _ = dijkstra_lengths(C)
    assert (S[allmiss] == 1).all()  # (an unassigned column always remains)
    assert (S[want7[:3]] == 1).all() and S[want7[3]] > 1
    c = small_ctx(sh, sd, wish)
    check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE)
    c.close()


def test_marker_rows_first(sh, small):
    """Rows with more than 32 hit columns (their entry 31 is the overflow
    marker) as first-step rows: one type on 40 columns, wanted by row 0, by
    rows in both halves of a tile dword and by the last row; few enough of
    them that the block's overflow list holds their entries."""
    from santa_hip import _lib
    sd, _ = small
    n = 256
    col_types = np.arange(n)
    held = np.random.default_rng(11).choice(n, 40, replace=False)
    col_types[held] = NG - 1  # (the wishlists' filler types stop short of it)
    rows_m = [0, 2, 3, 129, 255]
    free = np.setdiff1d(np.arange(n), held)  # (their types are their indices)
    heads = [[] if j in held else [int(col_types[j])] for j in range(n)]
    for j in rows_m:
        heads[j] = [NG - 1, int(free[(j + 1) % len(free)])]  # (and a second wish on one column)
    wish, types, rows = crafted(sd, col_types, heads)
    hits = (cost_v(wish[rows[0]], types[rows[0]]) < 0).sum(axis=1)
    assert (hits[rows_m] > 32).all() and (hits > 32).sum() == len(rows_m)
    assert int((hits[hits > 32] - 31).sum()) <= OVF_CAP
    c = small_ctx(sh, sd, wish)
    check_blocks(c, wish, sd.goodkids, types, rows, _lib.SH_FLAG_SP_TILE)
    c.close()


def test_real_states(sh, ctx, full_data):
    """64 blocks of the bench's round 0, and 64 blocks of its round 6 after
    six full rounds on the GPU, against the oracle from the same state."""
    from santa_hip import _lib
    mode, n, B = 0, 256, 64
    nb = ctx.geometry(mode, n)[3]
    rows0 = ctx.sample_blocks(mode, n, B, 2017, 0).cpu().numpy().reshape(B, n)
    check_blocks(ctx, full_data.wish, full_data.goodkids, full_data.types, rows0, _lib.SH_FLAG_SP_TILE,
                 apply=False)
    types = ctx.upload_types(full_data.types)
    for r in range(6):
        ctx.solve_blocks(mode, ctx.sample_blocks(mode, n, nb, 2017, r), n, types)
    t6 = types.cpu().numpy()
    rows6 = ctx.sample_blocks(mode, n, B, 2017, 6).cpu().numpy().reshape(B, n)
    ones = total = 0
    for b in range(0, B, 4):  # (the tracer is numpy: 16 of the 64 blocks)
        S, _ = dijkstra_lengths(cost_v(full_data.wish[rows6[b]], t6[rows6[b]]))
        ones += int((S == 1).sum())
        total += len(S)
    print("S = 1 share at round 6:", ones / total)
    assert 0.5 <= ones / total <= 0.9
    check_blocks(ctx, full_data.wish, full_data.goodkids, t6, rows6, _lib.SH_FLAG_SP_TILE, apply=False)


def test_unchanged_routing(sh, ctx, full_data):
    """SH_FLAG_TEST_RANGE and SH_FLAG_EXACT_ARGMIN still send every block to
    the fallback launch, with equal results; one SH_FLAG_TIMING launch returns."""
    from santa_hip import _lib
    mode, n, B = 0, 256, 8
    rows = ctx.sample_blocks(mode, n, B, 2017, 0)
    r = rows.cpu().numpy().reshape(B, n)
    for fl in (_lib.SH_FLAG_TEST_RANGE, _lib.SH_FLAG_EXACT_ARGMIN):
        check_blocks(ctx, full_data.wish, full_data.goodkids, full_data.types, r, _lib.SH_FLAG_SP_TILE | fl)
    types = ctx.upload_types(full_data.types)
    col = torch.zeros(B * n, dtype=torch.int32, device="cuda")
    steps = torch.zeros(B, dtype=torch.int64, device="cuda")
    ctx.solve_blocks(mode, rows, n, types, col=col, steps=steps,
                     flags=_lib.SH_FLAG_SP_TILE | _lib.SH_FLAG_TIMING | _lib.SH_FLAG_NO_APPLY)
    torch.cuda.synchronize()
    assert ctx.error_flags() == 0
    assert (col.view(B, n)[:, :7] >= 0).all()
