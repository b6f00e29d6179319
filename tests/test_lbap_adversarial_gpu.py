"""The bottleneck solver on the adversarial families of lbap_families.py: col
array-equal to the reference loop's (lbap_ref, live or recorded) and value
equal to it, bit for bit an entry of the instance where that says more, in
every kernel design that exists at the case's width.  No tolerances.

test_lbap_adversarial_cpu.py proves on the host what each family is for (the
nr-step search and nr-hop path, the wrong keys that would return another col)
and that CASES reaches all 60 lbap_kernels."""
import numpy as np
import pytest
import torch

import lbap_families as F
from lbap_ref import lbap_ref
from santa_hip import _lib, solve_bottleneck_batched
from test_lbap_gpu import check_against_refs, designs, solve, to_host

pytestmark = pytest.mark.gpu

CASES = F.CASES   # (family, dtype, nr, nc, maximize): each compares col with lbap_ref in every design


def to_torch(S, dt):
    """A stored matrix of lbap_families as a tensor of its dtype."""
    S = np.ascontiguousarray(S)
    return torch.from_numpy(S.view(np.int16)).view(torch.bfloat16) if dt == "bf16" else torch.from_numpy(S)


def value_bits(value, dt):
    return F.as_bits(value.view(torch.int16).numpy().view(np.uint16) if dt == "bf16" else value.numpy(), dt)


@pytest.mark.parametrize("case", CASES, ids=F.case_id)
def test_family(case):
    family, dt, nr, nc, maximize = case
    Cs, shapes, refs = F.batch(case)
    C = to_torch(Cs, dt)
    check_against_refs(C, refs, maximize=maximize, shapes=shapes)
    if family not in ("signed_zeros", "random_bits", "nan_patterns"):
        return
    # value bit for bit: an entry of the instance that the assignment chose
    # (an infeasible instance: the forbidden infinity itself)
    U = F.as_bits(Cs, dt)
    for name, flags in designs(nc):
        col, value = solve(C, flags, maximize=maximize)
        vb = value_bits(value, dt)
        for b, (rcol, rval) in enumerate(refs):
            if (rcol < 0).all():
                assert vb[b] == F.as_bits(F.store(np.array([rval], dtype=np.float64), dt), dt)[0], (name, b)
                continue
            assert vb[b] in U[b, np.arange(nr), col[b]], (name, b, vb[b])
            if family == "signed_zeros":
                assert int(vb[b]) & ~(1 << sum(F.LAYOUT[dt])) == 0, (name, b, vb[b])   # a zero of either sign


# --------------------------------------------------------------------------- smaller holes
@pytest.mark.parametrize("nr,nc,flag", [(65, 70, _lib.SH_FLAG_LBAP_SW), (300, 513, _lib.SH_FLAG_LBAP_MW)])
def test_without_value(nr, nc, flag):
    C = torch.from_numpy(np.stack([F.small_ints(nr, nc, k) for k in range(3)])).cuda()
    col, value = solve_bottleneck_batched(C, flags=flag)
    col2, none = solve_bottleneck_batched(C, with_value=False, flags=flag)
    torch.cuda.synchronize()
    assert none is None and value is not None
    assert torch.equal(col, col2)
    assert np.array_equal(col2[0].cpu().numpy(), lbap_ref(C[0].cpu().numpy())[0])


def test_70000_instances_in_the_multi_wave_design():
    """B beyond 65535 workgroups of four waves: the one-wave design's result
    on the same tensor (which test_lbap_gpu proves optimal), and a sample of 64
    against the reference."""
    B, n = 70000, 8
    rng = np.random.default_rng(18)
    Cb = rng.integers(np.iinfo(np.int32).min, np.iinfo(np.int32).max, size=(B, n, n), endpoint=True).astype(np.int32)
    Cb[::3] = rng.integers(0, 4, size=Cb[::3].shape)
    C = torch.from_numpy(Cb)
    assert F.config_of(n, B, _lib.SH_FLAG_LBAP_MW) == (4, 1)
    col, value = solve(C, _lib.SH_FLAG_LBAP_MW)
    col1, value1 = solve(C, _lib.SH_FLAG_LBAP_SW)
    assert np.array_equal(col, col1) and torch.equal(value, value1)
    for b in rng.choice(B, size=64, replace=False):
        rcol, rval, _, _ = lbap_ref(Cb[b])
        assert np.array_equal(col[b], rcol) and value.numpy()[b] == rval


@pytest.mark.parametrize("NR,NC", [(70, 70), (40, 300)])
@pytest.mark.parametrize("maximize", [False, True])
def test_ragged_16_bit_batches_never_read_the_padding(NR, NC, maximize):
    """test_lbap_gpu's ragged batch in float16 and bfloat16, the padding what
    would win if it were read, and NaN in a second run."""
    rng = np.random.default_rng([19, NR, NC])
    shapes = np.array([[0, 3], [1, 1], [NR, NC], [NR // 2, NC - 1], [0, 0], [3, NC]], dtype=np.int32)
    B = len(shapes)
    live = rng.integers(-128, 129, size=(B, NR, NC))
    inside = (np.arange(NR)[None, :, None] < shapes[:, 0, None, None]) & \
             (np.arange(NC)[None, None, :] < shapes[:, 1, None, None])
    refs = []
    for b, (r, c) in enumerate(shapes):
        col, value, _, _ = lbap_ref(live[b, :r, :c].astype(np.float64), maximize)
        refs.append((np.concatenate([col, np.full(NR - r, -1, dtype=np.int32)]), value))
    for dt in ("f16", "bf16"):
        assert np.array_equal(F.widen(F.store(live, dt), dt), live)
        for pad in (F.poison(dt, maximize), F.from_bits(F.nan_bits(dt), dt)[2]):
            Cs = F.store(np.where(inside, live, 0), dt)
            Cs[~inside] = pad
            check_against_refs(to_torch(Cs, dt), refs, maximize=maximize, shapes=shapes)


@pytest.mark.parametrize("nr,nc", [(65, 64), (300, 100)])
def test_tall_input_under_maximize(nr, nc):
    Cb = np.stack([F.small_ints(nr, nc, k) for k in range(2)]).astype(np.float32)
    want = []
    for b in range(2):
        col_t, rval, _, _ = lbap_ref(Cb[b].T, True)      # the row that each column takes
        w = np.full(nr, -1, dtype=np.int32)
        w[col_t] = np.arange(nc)
        want.append((w, rval))
    # (the transposed batch has nr columns: its designs)
    for name, flags in designs(nr):
        col, value = solve(torch.from_numpy(Cb), flags, maximize=True)
        for b, (w, rval) in enumerate(want):
            assert np.array_equal(col[b], w), (name, b)
            assert value.numpy()[b] == rval == Cb[b][col[b] >= 0, col[b][col[b] >= 0]].min()


def test_non_contiguous_input():
    rng = np.random.default_rng(20)
    base = torch.from_numpy(rng.integers(-1000, 1000, size=(3, 90, 140)).astype(np.int32)).cuda()
    for view in (base.transpose(1, 2),            # [3, 140, 90]: tall, strides (., 1, 140)
                 base.transpose(1, 2)[:, :60],    # [3, 60, 90]: wide
                 base[:, :, ::2],                 # [3, 90, 70]: tall, every other column
                 base[:, :40, ::2]):              # [3, 40, 70]: wide
        assert not view.is_contiguous()
        for name, flags in designs(max(view.shape[1:])):
            col, value = solve_bottleneck_batched(view, flags=flags)
            col_c, value_c = solve_bottleneck_batched(view.contiguous(), flags=flags)
            torch.cuda.synchronize()
            assert torch.equal(col, col_c) and torch.equal(value, value_c), name
        if view.shape[1] <= view.shape[2]:
            for b in range(3):
                rcol, rval, _, _ = lbap_ref(view[b].cpu().numpy())
                assert np.array_equal(col[b].cpu().numpy(), rcol) and value[b].item() == rval
