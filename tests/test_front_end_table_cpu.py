"""One table of bad calls and of empty batches, driven through all eight
batched front ends: the exception types and message texts, and the shapes,
dtypes and fill values of an empty batch's result.  Host only: the costs are
CPU tensors and every call here is answered before the GPU is asked for
(lsap.require_gpu is patched out, since the order of the two has differed
between the entries; lbap's stays real)."""
import numpy as np
import pytest
import torch

from santa_hip import lbap, lsap

I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
BASE = (2, 3, 4)


def _csr(shape, dtype=F64):
    """The full pattern of a [B, NR, NC] batch as (crow, col_indices, values)."""
    B, NR, NC = shape
    return (torch.arange(B * NR + 1, dtype=I64) * NC, torch.arange(NC, dtype=I32).repeat(B * NR),
            torch.ones(B * NR * NC, dtype=dtype))


class Entry:
    """One batched front end: its size limit, what it takes besides C, and a
    call with valid companions for a cost tensor of any (3-D) shape."""

    def __init__(self, name, limit, takes=None):
        self.name, self.limit, self.takes = name, limit, takes

    def companions(self, shape, dtype):
        B, NR, NC = shape
        ddt = F64 if dtype.is_floating_point else I64
        if self.takes == "duals":
            return dict(col=torch.zeros((B, NR), dtype=I32), u=torch.zeros((B, NR), dtype=ddt),
                        v=torch.zeros((B, NC), dtype=ddt))
        if self.takes == "witness":
            return dict(col=torch.zeros((B, NR), dtype=I32), value=torch.zeros(B, dtype=dtype),
                        wit=torch.zeros((B, min(NR, NC)), dtype=torch.uint8))
        return {}

    def __call__(self, C, shape=None, shapes=None, **over):
        """shape: the batch the companions are made for (default: C's own)."""
        if self.name == "solve_batched_sparse":
            shape = tuple(C.shape) if shape is None else shape
            crow, idx, val = _csr(shape if len(shape) == 3 else BASE, C.dtype)
            return lsap.solve_batched_sparse(crow, idx, val, shape=shape, shapes=shapes, duals=True)
        args = self.companions(tuple(C.shape) if shape is None else shape, C.dtype)
        args.update(over)
        f = getattr(lbap if "bottleneck" in self.name else lsap, self.name)
        if self.takes is None:
            extra = dict(witness=True) if "bottleneck" in self.name else dict(duals=True)
            return f(C, shapes=shapes, **extra)
        return f(C, *args.values(), shapes=shapes)


ENTRIES = [Entry("solve_batched", 1024), Entry("solve_batched_large", 4096),
           Entry("check_duals", 1024, "duals"), Entry("check_duals_large", 4096, "duals"),
           Entry("resolve_batched", 4096, "duals"), Entry("solve_batched_sparse", 4096),
           Entry("solve_bottleneck_batched", 4096), Entry("check_bottleneck", 4096, "witness")]


@pytest.fixture(autouse=True)
def no_gpu_needed(monkeypatch):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)


def _raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == text


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_bad_batches(entry):
    sparse = entry.name == "solve_batched_sparse"
    C = torch.zeros(BASE, dtype=I64 if not sparse else F64)
    # rank (the CSR entry's shape triple has its own words)
    if sparse:
        _raises(ValueError, "shape = (B, NR, NC) is required", lambda: entry(C, shape=BASE[1:]))
    else:
        _raises(ValueError, "expected [B, NR, NC]", lambda: entry(C[0], shape=BASE))
    # one above the size limit, wide and (the CSR entry is wide only) tall
    n = entry.limit + 1
    for shape in ((1, 2, n),) if sparse else ((1, 2, n), (1, n, 2)):
        big = torch.zeros((1, 1, 1), dtype=C.dtype).expand(shape)
        if sparse:  # (the limit is checked before crow is looked at: the base pattern will do)
            _raises(ValueError, f"max(NR, NC) = {n} > {entry.limit}",
                    lambda: lsap.solve_batched_sparse(*_csr(BASE), shape=shape))
        else:
            _raises(ValueError, f"max(NR, NC) = {n} > {entry.limit}", lambda: entry(big))
    # dtype (the CSR entry converts integer values to float64 and refuses complex ones)
    if sparse:
        _raises(TypeError, "unsupported dtype torch.complex64", lambda: entry(C.to(torch.complex64)))
    else:
        _raises(TypeError, "unsupported dtype torch.int16", lambda: entry(C.to(torch.int16)))
    # shapes
    tall = torch.zeros((2, 4, 3), dtype=C.dtype)
    if sparse:
        _raises(ValueError, "a sparse batch must be wide, got [4, 3]: transpose it so that NR <= NC",
                lambda: entry(tall, shapes=[[3, 3], [3, 3]]))
    else:
        _raises(ValueError, "a ragged batch must be padded wide, got [4, 3]: "
                "transpose the batch so that every instance has nr <= nc", lambda: entry(tall, shapes=[[3, 3], [3, 3]]))
    _raises(ValueError, "shapes[1] = (3, 2) is tall (nr > nc): transpose the batch so that every instance has nr <= nc",
            lambda: entry(C, shapes=[[3, 4], [3, 2]]))
    _raises(ValueError, "shapes[1] = (4, 4) is outside the padded [3, 4] matrix",
            lambda: entry(C, shapes=torch.tensor([[3, 4], [4, 4]])))
    _raises(ValueError, "shapes[0] = (-1, 4) is outside the padded [3, 4] matrix",
            lambda: entry(C, shapes=[[-1, 4], [3, 4]]))
    _raises(ValueError, "shapes must be an integer [B, 2] = [2, 2] array, got int64 (1, 2)",
            lambda: entry(C, shapes=np.array([[3, 4]])))
    _raises(ValueError, "shapes must be an integer [B, 2] = [2, 2] array, got float64 (2, 2)",
            lambda: entry(C, shapes=np.array([[3.0, 4.0], [3.0, 4.0]])))


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.takes == "duals"], ids=lambda e: e.name)
def test_bad_previous_solutions(entry):
    C = torch.zeros(BASE, dtype=I64)
    shape = "expected col and u of shape [2, 3] and v of shape [2, 4]"
    _raises(ValueError, shape, lambda: entry(C, col=torch.zeros((2, 4), dtype=I32)))
    _raises(ValueError, shape, lambda: entry(C, u=torch.zeros((2, 4), dtype=I64)))
    _raises(ValueError, shape, lambda: entry(C, v=torch.zeros((2, 3), dtype=I64)))
    _raises(ValueError, shape, lambda: entry(C, v=torch.zeros(4, dtype=I64)))
    _raises(TypeError, "the duals of torch.int64 costs are torch.int64",
            lambda: entry(C, u=torch.zeros((2, 3), dtype=F64), v=torch.zeros((2, 4), dtype=F64)))
    _raises(TypeError, "the duals of torch.float32 costs are torch.float64",
            lambda: entry(C.float(), v=torch.zeros((2, 4), dtype=F32)))
    _raises(TypeError, "col must be an integer tensor, got torch.float32",
            lambda: entry(C, col=torch.zeros((2, 3), dtype=F32)))


def test_bad_bottleneck_claims():
    entry = ENTRIES[-1]
    C = torch.zeros(BASE, dtype=F32)
    shape = "expected col [2, 3], value [2] and wit [2, 3]"
    _raises(ValueError, shape, lambda: entry(C, col=torch.zeros((2, 4), dtype=I32)))
    _raises(ValueError, shape, lambda: entry(C, value=torch.zeros((2, 1), dtype=F32)))
    _raises(ValueError, shape, lambda: entry(C, wit=torch.zeros((2, 4), dtype=torch.uint8)))
    _raises(ValueError, "expected col [2, 4], value [2] and wit [2, 3]",  # (a tall batch: wit over the columns)
            lambda: entry(C.transpose(1, 2), wit=torch.zeros((2, 4), dtype=torch.uint8)))
    _raises(TypeError, "value must be torch.float32 and wit uint8 or bool", lambda: entry(C, value=torch.zeros(2, dtype=F64)))
    _raises(TypeError, "value must be torch.float32 and wit uint8 or bool",
            lambda: entry(C, wit=torch.zeros((2, 3), dtype=I32)))
    _raises(TypeError, "col must be an integer tensor, got torch.float32",
            lambda: entry(C, col=torch.zeros((2, 3), dtype=F32)))


def _is(t, shape, dtype, fill):
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == tuple(shape) and t.dtype == dtype, (t, shape, dtype)
    assert t.device.type == "cpu" and bool((t == fill).all())


@pytest.mark.parametrize("shape", [(0, 3, 4), (2, 0, 4), (2, 3, 0)], ids=str)
@pytest.mark.parametrize("dtype", [I32, F32], ids=str)
def test_empty_batches(shape, dtype):
    B, NR, NC = shape
    ddt = F64 if dtype.is_floating_point else I64
    C = torch.zeros(shape, dtype=dtype)
    col0, u0, v0 = torch.zeros((B, NR), dtype=I64), torch.zeros((B, NR), dtype=ddt), torch.zeros((B, NC), dtype=ddt)

    def solved(out, cost_dtype, n):
        assert len(out) == n
        _is(out[0], (B, NR), I32, -1)
        _is(out[1], (B,), cost_dtype, 0)
        if n >= 4:
            _is(out[2], (B, NR), ddt, 0)
            _is(out[3], (B, NC), ddt, 0)

    for f in (lsap.solve_batched, lsap.solve_batched_large):
        solved(f(C), ddt, 2)
        solved(f(C, duals=True, maximize=True), ddt, 4)
        out = f(C, with_cost=False, shapes=np.zeros((B, 2), dtype=np.int64)) if NR <= NC else f(C, with_cost=False)
        assert len(out) == 2 and out[1] is None
        _is(out[0], (B, NR), I32, -1)
    for f in (lsap.check_duals, lsap.check_duals_large):
        out = f(C, col0, u0, v0, maximize=True)
        assert len(out) == 4
        for t in out[:3]:
            _is(t, (B,), ddt, 0)
        _is(out[3], (B,), I32, 0)
    out = lsap.resolve_batched(C, col0, u0, v0)
    solved(out, ddt, 5)
    _is(out[4], (B,), I32, 0)
    out = lsap.resolve_batched(C, col0, u0, v0, with_cost=False, maximize=True)
    assert len(out) == 5 and out[1] is None
    if NR <= NC:  # (the CSR entry is wide only; its values are solved as float64 whatever they were)
        crow = torch.zeros(B * NR + 1, dtype=I64)
        solved(lsap.solve_batched_sparse(crow, torch.zeros(0, dtype=I32), torch.zeros(0, dtype=dtype), shape=shape), F64, 2)
        out = lsap.solve_batched_sparse(crow, torch.zeros(0, dtype=I32), torch.zeros(0, dtype=dtype), shape=shape,
                                        duals=True, maximize=True)
        assert len(out) == 4
        _is(out[0], (B, NR), I32, -1)
        for t, s in zip(out[1:], ((B,), (B, NR), (B, NC))):
            _is(t, s, F64, 0)
    else:
        _raises(ValueError, f"a sparse batch must be wide, got [{NR}, {NC}]: transpose it so that NR <= NC",
                lambda: lsap.solve_batched_sparse(torch.zeros(B * NR + 1, dtype=I64), torch.zeros(0, dtype=I32),
                                                  torch.zeros(0, dtype=dtype), shape=shape))
    solved(lbap.solve_bottleneck_batched(C, maximize=True), dtype, 2)
    out = lbap.solve_bottleneck_batched(C, witness=True)
    solved(out, dtype, 3)
    _is(out[2], (B, min(NR, NC)), torch.uint8, 0)
    out = lbap.solve_bottleneck_batched(C, with_value=False)
    assert len(out) == 2 and out[1] is None
    out = lbap.check_bottleneck(C, col0, torch.zeros(B, dtype=dtype), torch.zeros((B, min(NR, NC)), dtype=torch.bool))
    assert len(out) == 3
    for t in out:
        _is(t, (B,), I32, 0)
