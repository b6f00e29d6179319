"""The Santa block kernels on contexts at the edges of their shape guards
(tests/ctx_shapes.py): one context on each side of every guard of
csrc/santa_api.inc, every kernel design on each of them, against the CPU
oracle bit for bit (col, exact cost, the whole type vector, steps, deltas).

There are two outcomes for a call: it solves the round as the oracle does,
or -- a forced design only -- it is refused (ValueError with the library's
text, types untouched, no error flag, the context still good).  The default
dispatch must solve every shape sh_ctx_create accepted.

Each test prints what it resolved (`CTXSHAPE ...` lines, visible with -s):
the design per (shape, mode, n, flags), refusals with their text, and the
blocks that took the fallback launch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ctx_shapes as CS  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

FORCED = CS.F_LDS | CS.F_VT | CS.F_SP | CS.F_SP1 | CS.F_DT | CS.F_BIG
EXTRA_CASES = {"ng4000": [(0, 1025, 1, (0,))],  # the staged-row kernel's LDS guard, other side
               # the twins tile's LDS guard: the last n that fits and the first that does not
               "ng8192": [(1, 243, 2, (0, CS.F_RANGE)), (1, 244, 2, (0, CS.F_RANGE))]}


@pytest.fixture(scope="module")
def ctxs():
    """name -> the shape's context, created on first use, all closed at the end."""
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    made = {}

    def get(name):
        if name not in made:
            made[name] = santa_hip.SantaGPU.from_data(CS.data(name), 0)
        return made[name]

    yield get
    for c in made.values():
        c.close()


_WANT = {}


def want_round(name, mode, rows, tag):
    """The oracle's round over rows [B, n] from the shape's baseline, computed
    once per (shape, mode, tag) and shared."""
    key = (name, mode, tag)
    if key not in _WANT:
        sd = CS.data(name)
        t = sd.types.copy()
        st = np.zeros(2, dtype=np.uint64)
        col, cost = oracle.round_blocks(mode, sd.wish, t, rows, stats=st, ng=sd.ng)
        s0 = base_sums(name)
        s1 = oracle.score_sums(sd.wish, sd.goodkids, t)
        moved = int((col != np.arange(rows.shape[1])).sum())
        assert moved >= rows.size // 2, (key, moved)  # (no trivial identity round)
        _WANT[key] = dict(rows=rows.copy(), col=col, cost=cost, types=t, steps=int(st[0]),
                          delta=[s1[0] - s0[0], s1[1] - s0[1]], sums=s1)
    assert np.array_equal(_WANT[key]["rows"], rows), key
    return _WANT[key]


def base_sums(name):
    key = (name, "base")
    if key not in _WANT:
        sd = CS.data(name)
        _WANT[key] = oracle.score_sums(sd.wish, sd.goodkids, sd.types)
    return _WANT[key]


def solve(ctx, sd, mode, rows, n, B, fl):
    """-> (outputs, None), or (types, text) when the library refuses the call."""
    from santa_hip import _lib
    types = ctx.upload_types(sd.types)
    col = torch.full((B * n,), -1, dtype=torch.int32, device="cuda")
    cost = torch.zeros(B, dtype=torch.int64, device="cuda")
    delta = torch.zeros(2, dtype=torch.int64, device="cuda")
    steps = torch.zeros(B, dtype=torch.int64, device="cuda")
    try:
        ctx.solve_blocks(mode, rows, n, types, col=col, cost=cost, delta=delta, steps=steps, flags=fl)
    except ValueError:
        return types, _lib.last_error()
    return dict(col=col.cpu().numpy().reshape(B, n), cost=cost.cpu().numpy(), types=types.cpu().numpy(),
                steps=int(steps.sum()), delta=delta.cpu().tolist()), None


def assert_matches(got, want, what):
    assert np.array_equal(got["col"], want["col"]), what
    assert np.array_equal(got["cost"], want["cost"]), what
    assert np.array_equal(got["types"], want["types"]), what
    assert got["steps"] == want["steps"], what
    assert got["delta"] == want["delta"], what


def run_case(ctx, name, mode, rows_np, n, B, flag_sets, tag):
    """Every flag set of one (mode, n, B) on one block set: the design is the
    guards', the result the oracle's -- or a forced design's clean refusal."""
    sd = CS.data(name)
    s = CS.BY_NAME[name]
    want = want_round(name, mode, rows_np, tag)
    rows = torch.from_numpy(np.ascontiguousarray(rows_np.reshape(-1))).cuda()
    for fl in flag_sets:
        what = (name, mode, n, B, fl, tag)
        design = ctx.solve_design(mode, n, B, fl)
        exp = CS.expected_design(s, mode, n, fl)
        assert design in exp if isinstance(exp, set) else design == exp, (what, design, exp)
        got, refused = solve(ctx, sd, mode, rows, n, B, fl)
        print(f"CTXSHAPE design {name} mode={mode} n={n} B={B} flags={fl} {tag}: {design}"
              + (f" REFUSED: {refused}" if refused is not None else f" fallback_blocks={ctx.fallback_blocks()}"))
        if refused is not None:
            assert fl & FORCED, (what, "the default dispatch refused", refused)
            assert refused, what
            assert np.array_equal(got.cpu().numpy(), sd.types), what
            assert ctx.error_flags() == 0, what
            got, again = solve(ctx, sd, mode, rows, n, B, 0)  # the context is still good
            assert again is None, (what, again)
        assert_matches(got, want, what)
        assert ctx.error_flags() == 0, what


@pytest.mark.parametrize("name", CS.NAMES)
def test_sampled_blocks_match_oracle(ctxs, name):
    ctx = ctxs(name)
    s = CS.BY_NAME[name]
    cases = CS.CASES + [(2, CS.triplet_block_n(s), 1, (0,))] + EXTRA_CASES.get(name, [])
    for mode, n, B, flag_sets in cases:
        rows = ctx.sample_blocks(mode, n, B, 2024, 1).cpu().numpy().reshape(B, n)
        run_case(ctx, name, mode, rows, n, B, flag_sets, ("sampled", n, B))


@pytest.mark.parametrize("name", CS.NAMES)
def test_hand_built_blocks_match_oracle(ctxs, name):
    """The lowest singles ids and (nc2p20, nc_over) the highest child ids,
    nc - 1 included: the ids the 20-bit child fields exist for."""
    ctx = ctxs(name)
    s = CS.BY_NAME[name]
    for n, flag_sets in ((256, CS.SINGLES_256_FLAGS), (600, (0, CS.F_BIG, CS.F_RANGE))):
        rows = CS.hand_blocks(s, n)
        run_case(ctx, name, 0, rows, n, rows.shape[0], flag_sets, ("hand", n))


def test_design_pins(ctxs):
    """Each guard's constant, from both sides (the table is written from the
    guards' text: a mismatch is a finding about the guard or about the table)."""
    for name, mode, n, B, fl, want in CS.PINS:
        assert ctxs(name).solve_design(mode, n, B, fl) == want, (name, mode, n, B, fl)


@pytest.mark.parametrize("name", CS.NAMES)
def test_score_matches_oracle(ctxs, name):
    """sh_score on the baseline and after a singles and a twins round (the
    n_good = 1 shape and nc_over included)."""
    ctx = ctxs(name)
    sd = CS.data(name)
    types = ctx.upload_types(sd.types)
    assert ctx.score_sums(types) == base_sums(name)
    for mode, n, B in ((0, 256, 8), (1, 256, 2)):
        ctx.solve_blocks(mode, ctx.sample_blocks(mode, n, B, 2024, 1), n, types)
    t = types.cpu().numpy()
    assert not np.array_equal(t, sd.types)
    got = ctx.score_sums(types)
    assert got == oracle.score_sums(sd.wish, sd.goodkids, t)
    assert got[2] == 0 and got[3] == 0 and got[:2] != base_sums(name)[:2]
    assert ctx.error_flags() == 0


@pytest.mark.parametrize("name", ["nw126", "nw127"])
def test_longest_wishlists_run_the_sparse_solvers(ctxs, name):
    """At n_wish = 126, 127 and 200 gift types a 256-column block has ~160
    hits per row: the sparse designs leave such blocks to their fallback
    launch for capacity, and the 7-bit wish code would never be solved with.
    Blocks of 40 columns (~25 hits per row) fit, so the register-tile sparse
    kernel (n_wish = 126: wish values up to 126 in its 7-bit field) and the
    LDS-list kernel (127) solve them themselves: the blocks they leave are
    exactly those the capacities predict (none, here)."""
    ctx = ctxs(name)
    sd = CS.data(name)
    mode, n, B = 0, 40, 4
    rows = ctx.sample_blocks(mode, n, B, 2024, 1)
    rows_np = rows.cpu().numpy().reshape(B, n)
    want = want_round(name, mode, rows_np, ("sampled", n, B))
    list_cap = ctx.set_sparse_budget(0)
    for fl, design in ((CS.F_SP, CS.SPARSE3 if name == "nw126" else CS.SPARSE), (CS.F_SP1, CS.SPARSE)):
        assert ctx.solve_design(mode, n, B, fl) == design
        left = (CS.sparse_blocks_left(sd, rows_np, 512, None) if design == CS.SPARSE3
                else CS.sparse_blocks_left(sd, rows_np, None, list_cap))
        assert left == 0, (name, fl, left)  # (the case exists to run the primary solver)
        got, refused = solve(ctx, sd, mode, rows, n, B, fl)
        assert refused is None, refused
        fb = ctx.fallback_blocks()
        print(f"CTXSHAPE sparse {name} n={n} flags={fl} design={design}: {fb} of {B} blocks left, "
              f"hits per row {CS.block_hits(sd, rows_np[0]).mean():.1f}, list capacity {list_cap}")
        assert_matches(got, want, (name, fl))
        assert fb == left, (name, fl, fb)
    assert ctx.error_flags() == 0


LATTICE_DESIGNS = (CS.DT_TILE, CS.SPARSE3, CS.VT_TILE, CS.LARGE_LB)  # primary launch in 32-bit lattice units


@pytest.mark.parametrize("name", ["nw1", "nw2", "nw3"])
def test_natural_fallback(ctxs, name):
    """The lattice box at its smallest.  n_wish = 1 gives M = 1: no box, so
    every design whose primary launch solves in lattice units (dense tile,
    register-tile sparse, 4-wave register tile, staged-row) must send every
    singles block to its fallback launch by itself: fallback_blocks() == B.
    The LDS-list sparse kernel solves in exact 64-bit units and leaves blocks
    for capacity only (none here).  The round equals the oracle's either way.

    At n_wish = 2, 3 (M = 3, 5) whether real blocks leave the box was not
    known; the counts are printed and carried in the assertion messages, not
    asserted.  Measured on an MI355X (8 blocks of 256, 2 of 600): n_wish = 2
    -- the 4-wave register tile left all 8 (its solver, sap_solve_mw_l32,
    allows the column duals no miss part at M = 3), every other design none;
    n_wish = 3 -- none on any design.

    sh_ctx_fallback_steps is printed beside them and was 0 everywhere, at
    n_wish = 1 too: it counts steps of the windowed-key solver that needed
    the exact two-pass argmin (cost spreads beyond 2^42 units), not blocks
    solved by a fallback launch, so it cannot show that a block took one;
    sh_ctx_fallback_blocks does."""
    ctx = ctxs(name)
    sd = CS.data(name)
    ctx.fallback_steps()
    list_cap = ctx.set_sparse_budget(0)
    seen = []
    for mode, n, B, fl in ((0, 256, 8, 0), (0, 256, 8, CS.F_SP), (0, 256, 8, CS.F_SP1), (0, 256, 8, CS.F_VT),
                           (0, 256, 8, CS.F_DT), (0, 600, 2, 0)):
        rows = ctx.sample_blocks(mode, n, B, 2024, 1)
        rows_np = rows.cpu().numpy().reshape(B, n)
        want = want_round(name, mode, rows_np, ("sampled", n, B))
        design = ctx.solve_design(mode, n, B, fl)
        got, refused = solve(ctx, sd, mode, rows, n, B, fl)
        assert refused is None, (name, n, fl, refused)
        fb, st = ctx.fallback_blocks(), ctx.fallback_steps()
        seen.append(dict(n=n, flags=fl, design=design, left=fb, B=B, exact_steps=st))
        print(f"CTXSHAPE fallback {name} n={n} flags={fl} design={design}: {fb} of {B} blocks, "
              f"{st} exact-argmin steps")
        assert_matches(got, want, (name, seen))
        assert 0 <= fb <= B, (name, seen)
        if design == CS.SPARSE:
            assert fb == CS.sparse_blocks_left(sd, rows_np, None, list_cap), (name, seen)
        elif name == "nw1":
            assert design in LATTICE_DESIGNS and fb == B, (name, seen)
    assert {d["design"] for d in seen} >= {CS.SPARSE3, CS.SPARSE, CS.VT_TILE, CS.DT_TILE, CS.LARGE_LB}
    # a design without a fallback launch reports none
    rows = ctx.sample_blocks(1, 256, 2, 2024, 1)
    solve(ctx, sd, 1, rows, 256, 2, 0)
    assert ctx.fallback_blocks() == 0
    assert ctx.error_flags() == 0


def test_forced_design_refusal_is_clean(ctxs):
    """A forced design that cannot launch is refused, nothing else: the
    LDS-list sparse kernel under a hit-list budget of 100 KiB needs more than
    the 64 KiB it may ask for.  ValueError with the library's text, the types
    bit for bit untouched, no error flag, and the next default call on the
    same context still equals the oracle."""
    from santa_hip import _lib
    name, mode, n, B = "ng1022", 0, 256, 8
    ctx = ctxs(name)
    sd = CS.data(name)
    rows = ctx.sample_blocks(mode, n, B, 2024, 1)
    want = want_round(name, mode, rows.cpu().numpy().reshape(B, n), ("sampled", n, B))
    try:
        assert ctx.set_sparse_budget(100 * 1024) > 0
        assert ctx.solve_design(mode, n, B, CS.F_SP1) == CS.SPARSE
        types = ctx.upload_types(sd.types)
        with pytest.raises(ValueError, match="64 KiB"):
            ctx.solve_blocks(mode, rows, n, types, flags=CS.F_SP1)
        assert "64 KiB" in _lib.last_error()
        assert np.array_equal(types.cpu().numpy(), sd.types)
        assert ctx.error_flags() == 0
        got, refused = solve(ctx, sd, mode, rows, n, B, 0)
        assert refused is None
        assert_matches(got, want, "default after a refusal")
    finally:
        ctx.set_sparse_budget(0)
    got, refused = solve(ctx, sd, mode, rows, n, B, CS.F_SP1)
    assert refused is None
    assert_matches(got, want, "the forced design at its default budget")
    assert ctx.error_flags() == 0


@pytest.mark.parametrize("name,fl,hand", [("ng1023", 0, False), ("nw127", 0, False), ("nw127", CS.F_SP, False),
                                          ("nw1", 0, False), ("nw1", CS.F_SP, False), ("nc_over", 0, True)])
def test_solve_round_bookkeeping_at_the_edges(ctxs, name, fl, hand):
    """sh_solve_round where the primary launch is the register tile (ng1023,
    nc_over with the highest child ids), the LDS-list sparse kernel (nw127,
    forced at this B) and where every block is solved by the fallback launch,
    which neither records nor samples (nw1): the assertions of
    test_solve_round_bookkeeping."""
    ctx = ctxs(name)
    sd = CS.data(name)
    s = CS.BY_NAME[name]
    mode, n, B = 0, 256, 8
    _, _, _, nb = ctx.geometry(mode, n)
    nb = min(nb, 64)
    if hand:
        sampled = ctx.sample_blocks(mode, n, B + 1, 77, 3).cpu().numpy()
        rows_np = CS.merge_blocks(CS.hand_blocks(s, n), sampled, B)
        assert sd.nc - 1 in rows_np
    else:
        rows_np = ctx.sample_blocks(mode, n, B, 77, 3).cpu().numpy().reshape(B, n)
    rows = torch.from_numpy(rows_np.reshape(-1)).cuda()
    want = want_round(name, mode, rows_np, ("round", n, B))
    design = ctx.solve_design(mode, n, B, fl)
    if name in ("ng1023", "nc_over"):
        assert design == CS.VT_TILE
    if name == "nw127" and fl:
        assert design == CS.SPARSE
    seq = (1 << 41) + 16 * CS.NAMES.index(name) + (fl != 0)
    mail = ctx.mailbox
    outs = []
    for fused in (False, True):
        types = ctx.upload_types(sd.types)
        col = torch.empty(B * n, dtype=torch.int32, device="cuda")
        cost = torch.empty(B, dtype=torch.int64, device="cuda")
        delta = torch.zeros(2, dtype=torch.int64, device="cuda")
        if fused:
            undo = torch.full((B * n,), -7, dtype=torch.int16, device="cuda")
            nxt = torch.full((nb * n,), -1, dtype=torch.int32, device="cuda")
            ctx.solve_round(mode, rows, n, types, undo=undo, next_round=(77, 4, nb, nxt), col=col, cost=cost,
                            delta=delta, publish=(1, seq), flags=fl)
            torch.cuda.synchronize()
            assert mail[4] == seq
            assert delta.cpu().tolist() == [0, 0]
            delta = torch.tensor([mail[5], mail[6]], dtype=torch.int64)
            if name == "nw1":
                assert ctx.fallback_blocks() == B
        else:
            ctx.solve_blocks(mode, rows, n, types, col=col, cost=cost, delta=delta, flags=fl)
        assert ctx.error_flags() == 0
        outs.append([x.cpu().numpy() for x in (col, cost, delta, types)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    assert np.array_equal(outs[1][0].reshape(B, n), want["col"])
    assert np.array_equal(outs[1][1], want["cost"])
    assert outs[1][2].tolist() == want["delta"]
    assert np.array_equal(outs[1][3], want["types"])
    assert np.array_equal(undo.cpu().numpy(), sd.types[rows_np.reshape(-1)])
    assert np.array_equal(nxt.cpu().numpy(), ctx.sample_blocks(mode, n, nb, 77, 4).cpu().numpy())
    types = torch.from_numpy(outs[1][3]).cuda()
    ctx.unpack_types(types, rows, undo, mode)
    assert np.array_equal(types.cpu().numpy(), sd.types)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", CS.HIGH_ID_SHAPES)
def test_undo_record_restores_the_baseline(ctxs, name, mode):
    """sh_sample_blocks_undo, a round, sh_unpack_types: the baseline comes
    back bit for bit; singles also with the highest child ids in the round
    (the undo record written by the block kernels)."""
    ctx = ctxs(name)
    sd = CS.data(name)
    s = CS.BY_NAME[name]
    n = 256 if mode < 2 else CS.triplet_block_n(s)
    B = 2
    types = ctx.upload_types(sd.types)
    rows = torch.empty(B * n, dtype=torch.int32, device="cuda")
    undo = torch.full((B * n,), -7, dtype=torch.int16, device="cuda")
    ctx.sample_blocks_undo(mode, n, B, 31, 2, types, rows, undo)
    assert torch.equal(rows, ctx.sample_blocks(mode, n, B, 31, 2))
    r = rows.cpu().numpy()
    assert np.array_equal(undo.cpu().numpy(), sd.types[r])
    ctx.solve_blocks(mode, rows, n, types)
    assert not np.array_equal(types.cpu().numpy(), sd.types)
    ctx.unpack_types(types, rows, undo, mode)
    assert np.array_equal(types.cpu().numpy(), sd.types)
    if mode == 0:
        hb = CS.hand_blocks(s, n)
        rows = torch.from_numpy(hb.reshape(-1)).cuda()
        undo = torch.full((hb.size,), -7, dtype=torch.int16, device="cuda")
        ctx.solve_round(mode, rows, n, types, undo=undo)
        t1 = types.cpu().numpy()
        assert np.array_equal(t1, want_round(name, 0, hb, ("hand", n))["types"])
        assert t1[sd.nc - 1] != sd.types[sd.nc - 1] or (t1[hb[1]] != sd.types[hb[1]]).sum() >= n // 2
        assert np.array_equal(undo.cpu().numpy(), sd.types[hb.reshape(-1)])
        ctx.unpack_types(types, rows, undo, mode)
        assert np.array_equal(types.cpu().numpy(), sd.types)
    assert ctx.error_flags() == 0
