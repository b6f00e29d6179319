"""Every batched front end on the smallest batches that have a tall case, a
square case without shapes (the square C form), an empty instance and a full
corner, with the costs given in three memory layouts: the results are the same
bits, no input is written, and each solve passes its own certificate."""
import numpy as np
import pytest
import torch

from santa_hip import (check_bottleneck, check_duals, check_duals_large, resolve_batched, solve_batched,
                       solve_batched_large, solve_batched_sparse, solve_bottleneck_batched)

pytestmark = pytest.mark.gpu

B = 3
RAGGED = [(0, 0), (3, 7), (5, 5)]
CASES = [(5, 7, None), (7, 5, None), (5, 5, None), (5, 7, RAGGED)]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    """Two results (tuples of tensors or None) with the same bits."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _layouts(C):
    """C three ways -> [(view, the tensor that owns its memory)]: contiguous, a
    transposed view of a contiguous [B, NC, NR] tensor, and every second
    instance of a [2B, NR, NC] tensor whose other instances hold other values."""
    t = C.transpose(1, 2).contiguous()
    big = torch.full((2 * C.shape[0],) + tuple(C.shape[1:]), 3, dtype=C.dtype, device=C.device)
    big[::2] = C
    return [(C.contiguous(), C), (t.transpose(1, 2), t), (big[::2], big)]


class Untouched:
    """The tensors handed to a call are bit-equal to their clones afterwards."""

    def __init__(self, *tensors):
        self.tensors = tensors
        self.before = [t.clone() for t in tensors]

    def check(self):
        for t, c in zip(self.tensors, self.before):
            assert torch.equal(_bits(t), _bits(c))


@pytest.mark.parametrize("maximize", [False, True], ids=["min", "max"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.float32], ids=["i32", "f32"])
@pytest.mark.parametrize("NR,NC,shapes", CASES, ids=["5x7", "7x5", "5x5", "5x7ragged"])
def test_layouts_agree_inputs_stay_and_round_trips_certify(NR, NC, shapes, dtype, maximize):
    rng = np.random.default_rng(NR * 100 + NC)
    Ci = torch.from_numpy(rng.integers(-20, 30, size=(B, NR, NC)).astype(np.int32)).cuda()
    C0 = Ci if dtype == torch.int32 else Ci.to(torch.float32) * 0.5  # (halves: exact in every float width)
    kw = dict(shapes=shapes, maximize=maximize)
    live_rows = torch.tensor([s[0] for s in shapes] if shapes else [min(NR, NC)] * B, dtype=torch.int32).cuda()
    results = []
    for C, owner in _layouts(C0):
        assert torch.equal(C, C0)
        res = {}
        keep = Untouched(owner)
        res["solve"] = solve_batched(C, duals=True, **kw)
        res["plain"] = solve_batched(C, **kw)
        res["large"] = col, cost, u, v = solve_batched_large(C, duals=True, **kw)
        _same(res["plain"], res["solve"][:2])
        _same(res["large"], res["solve"])  # (up to SH_MAX_N the large entry returns solve_batched's bits)
        sol = Untouched(col, u, v)
        res["check"] = check_duals(C, col, u, v, **kw)
        res["check_large"] = check_duals_large(C, col.long(), u, v, **kw)
        res["resolve"] = rcol, _, ru, rv, kept = resolve_batched(C, col, u, v, **kw)
        assert torch.equal(kept, live_rows) and torch.equal(rcol, col)  # every pair of the solution survives
        if dtype == torch.int32:  # integer certificates are exact
            assert not res["check"][3].any() and not res["check_large"][3].any()
            assert not check_duals_large(C, rcol, ru, rv, **kw)[3].any()
        sol.check()
        if NR <= NC:  # the CSR entry is wide only: the full pattern, values in this layout's order
            crow = torch.arange(B * NR + 1, dtype=torch.int64, device="cuda") * NC
            idx = torch.arange(NC, dtype=torch.int32, device="cuda").repeat(B * NR)
            csr = Untouched(crow, idx)
            res["sparse"] = solve_batched_sparse(crow, idx, C.reshape(-1), shape=(B, NR, NC), duals=True, **kw)
            _same(res["sparse"], solve_batched_large(C.double(), duals=True, **kw))
            csr.check()
        res["lbap"] = bcol, value, wit = solve_bottleneck_batched(C, witness=True, **kw)
        _same(solve_bottleneck_batched(C, **kw), res["lbap"][:2])
        claim = Untouched(bcol, value, wit)
        res["lbap_check"] = check_bottleneck(C, bcol, value, wit, **kw)
        assert not res["lbap_check"][2].any()
        claim.check()
        keep.check()
        results.append(res)
    for other in results[1:]:
        assert other.keys() == results[0].keys()
        for name in other:
            _same(other[name], results[0][name])
