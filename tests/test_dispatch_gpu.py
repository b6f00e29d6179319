"""The host dispatch's shared state: the overflow counter pair that every
design with a fallback launch alternates on, and the occupancy path's caches
(the dense-tile count per n, the dynamic-LDS attribute per kernel)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sh():
    import santa_hip
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    return santa_hip


@pytest.fixture(scope="module")
def ctx(sh, full_data):
    return sh.SantaGPU.from_data(full_data, 0)


def _round_outputs(ctx, full_data, rows, n, B, flags):
    types = ctx.upload_types(full_data.types)
    col = torch.empty(B * n, dtype=torch.int32, device="cuda")
    cost = torch.empty(B, dtype=torch.int64, device="cuda")
    delta = torch.zeros(2, dtype=torch.int64, device="cuda")
    steps = torch.empty(B, dtype=torch.int64, device="cuda")
    ctx.solve_blocks(0, rows, n, types, col=col, cost=cost, delta=delta, steps=steps, flags=flags)
    return [x.cpu().numpy() for x in (col, cost, delta, steps, types)]


def test_fallback_counters_shared_across_designs(sh, ctx, full_data):
    """An odd number of consecutive singles calls on one context that alternate
    the designs sharing the overflow counter pair, every block taking the
    fallback launch in one call and none in the next: each call equals the
    round of a design without a fallback launch (the 4-wave LDS tile at
    n = 64, the row-rebuild kernel at n = 300, the staged-row kernel's
    smallest configuration)."""
    from santa_hip import _lib as L
    B = 5
    rows = {n: ctx.sample_blocks(0, n, B, 77, 9) for n in (64, 300)}
    want = {64: _round_outputs(ctx, full_data, rows[64], 64, B, L.SH_FLAG_LDS_TILE),
            300: _round_outputs(ctx, full_data, rows[300], 300, B, L.SH_FLAG_BIG_ROWS)}
    assert ctx.solve_design(0, 64, B, L.SH_FLAG_LDS_TILE) == L.SH_DESIGN_LDS_TILE
    assert ctx.solve_design(0, 300, B, L.SH_FLAG_BIG_ROWS) == L.SH_DESIGN_LARGE
    # (n, flags, sparse budget, design): all blocks / no block to the fallback, in turn
    calls = [(64, L.SH_FLAG_SP_TILE | L.SH_FLAG_TEST_RANGE, 0, L.SH_DESIGN_SPARSE3),
             (64, L.SH_FLAG_DT_TILE, 0, L.SH_DESIGN_DT_TILE),
             (300, L.SH_FLAG_TEST_RANGE, 0, L.SH_DESIGN_LARGE_LB),
             (64, L.SH_FLAG_VT_TILE | L.SH_FLAG_TEST_RANGE, 0, L.SH_DESIGN_VT_TILE),
             (64, L.SH_FLAG_SP1, 16, L.SH_DESIGN_SPARSE),
             (64, L.SH_FLAG_SP_TILE, 0, L.SH_DESIGN_SPARSE3),
             (300, 0, 0, L.SH_DESIGN_LARGE_LB)]
    assert len(calls) % 2 == 1
    try:
        for k, (n, fl, budget, design) in enumerate(calls):
            assert ctx.solve_design(0, n, B, fl) == design, k
            assert ctx.set_sparse_budget(budget) >= 0
            got = _round_outputs(ctx, full_data, rows[n], n, B, fl)
            for name, x, y in zip(("col", "cost", "delta", "steps", "types"), want[n], got):
                assert np.array_equal(x, y), (k, name)
        assert ctx.error_flags() == 0
    finally:
        ctx.set_sparse_budget(0)


def test_occupancy_caches(sh, ctx, full_data):
    """sh_resident_blocks at another n in between leaves the count at n = 256
    and the picked designs as they were, for the dense tile (its count is
    cached per n) and the 4-wave LDS tile; and a query at a smaller n above
    64 KiB of LDS does not lower the attribute a later launch at n = 256 needs."""
    from santa_hip import _lib as L
    shapes = [(0, 256, 466, 0), (0, 256, 3730, 0), (0, 100, 466, 0), (0, 256, 466, L.SH_FLAG_LDS_TILE),
              (1, 256, 78, 0), (0, 2000, 477, 0)]
    designs = [ctx.solve_design(*s) for s in shapes]
    B = 5
    rows = ctx.sample_blocks(0, 256, B, 77, 9)
    for fl in (L.SH_FLAG_DT_TILE, L.SH_FLAG_LDS_TILE):
        before = _round_outputs(ctx, full_data, rows, 256, B, fl)
        first = ctx.resident_blocks(0, 256, 466, fl)
        assert first > 0
        assert ctx.resident_blocks(0, 100, 466, fl) >= first  # (less LDS per block)
        assert ctx.resident_blocks(0, 256, 466, fl) == first
        assert ctx.resident_blocks(0, 250, 466, fl) >= first
        after = _round_outputs(ctx, full_data, rows, 256, B, fl)
        for x, y in zip(before, after):
            assert np.array_equal(x, y), fl
    assert [ctx.solve_design(*s) for s in shapes] == designs
    assert ctx.error_flags() == 0
