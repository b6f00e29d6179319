"""Bottleneck assignment without a GPU: the host reference against an
independent threshold search, the library surface (exports, signatures, the
front ends' argument errors) and the lbap_ kernels' metadata."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from lbap_ref import lbap_ref, threshold_value
from santa_hip import _lib
from test_kernel_resources_cpu import _kernel_meta

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
I64 = np.iinfo(np.int64)


def _instances():
    """(C, maximize): 320 seeded instances up to 16 columns."""
    rng = np.random.default_rng(2024)
    for t in range(320):
        nc = int(rng.integers(1, 17))
        nr = int(rng.integers(1, nc + 1))
        kind = t % 8
        if kind == 0:
            yield rng.integers(0, 4, size=(nr, nc)).astype(np.int64), False          # ties in {0..3}
        elif kind == 1:
            yield rng.integers(-50, 50, size=(nr, nc)).astype(np.int32), bool(t & 8)  # negatives
        elif kind == 2:
            C = rng.random((nr, nc))
            C[rng.random((nr, nc)) < 0.5] = np.inf                                   # about 50 % +inf
            yield C, False
        elif kind == 3:
            yield np.outer(np.arange(1, nr + 1), np.arange(1, nc + 1)).astype(np.float64), bool(t & 8)  # product
        elif kind == 4:
            C = rng.integers(-3, 4, size=(nr, nc)).astype(np.int64)
            C[rng.random((nr, nc)) < 0.2] = I64.min
            C[rng.random((nr, nc)) < 0.2] = I64.max
            yield C, True                                                            # maximize on integers
        elif kind == 5:
            C = rng.integers(0, 4, size=(nr, nc)).astype(np.float32)
            C[rng.random((nr, nc)) < 0.3] = -np.inf
            C[rng.random((nr, nc)) < 0.1] = np.inf
            yield C, True                                                            # -inf forbidden, +inf best
        elif kind == 6:
            C = rng.integers(I64.min, I64.max, size=(nr, nc), endpoint=True)
            yield C, bool(t & 8)                                                     # the whole int64 range
        else:
            C = rng.integers(0, 3, size=(nr, nc)).astype(np.float64)
            C[rng.random((nr, nc)) < 0.15] = np.nan                                  # NaN is forbidden
            C[C == 0] = -0.0
            yield C, bool(t & 8)


def test_reference_loop_equals_threshold_search():
    n = infeasible = 0
    for C, maximize in _instances():
        col, value, _, _ = lbap_ref(C, maximize)
        want = threshold_value(C, maximize)
        n += 1
        assert value == want, (C, maximize, value, want)
        if (col < 0).any():
            infeasible += 1
            assert (col == -1).all() and np.isinf(value) and (value < 0) == maximize
            continue
        nr, nc = C.shape
        assert np.unique(col).size == nr and col.min() >= 0 and col.max() < nc
        chosen = C[np.arange(nr), col]
        assert (chosen.min() if maximize else chosen.max()) == value
    assert n >= 300 and 10 <= infeasible <= n // 2


def test_library_exports_the_six_entries_with_the_header_signatures():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "santa_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for suf in SUFFIXES:
        name = "lbap_solve_" + suf
        assert hasattr(L, name), name
        res, args = _lib.SIGNATURES[name]
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, f"{name} is not declared in santa_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(args) == 9
        for p, a in zip(params, args):
            want = _lib._P if "*" in p else _lib._U if p.startswith("unsigned") else _lib._I
            assert a is want, (name, p, a)
    for flag, bit in (("SH_FLAG_MAXIMIZE", 65536), ("SH_FLAG_LBAP_MW", 131072), ("SH_FLAG_LBAP_SW", 262144)):
        assert getattr(_lib, flag) == bit
        assert re.search(r"#define %s %du\b" % (flag, bit), header)


def test_c_abi_checks_its_arguments_before_any_device_call():
    """Every refusal is SH_ERR_ARGS with a text; none of them needs a GPU."""
    L = _lib.lib()
    fake = 4096  # a non-null pointer that is never dereferenced
    for suf in SUFFIXES:
        f = getattr(L, "lbap_solve_" + suf)
        for nr, nc, B, C, col, flags in ((0, 4, 1, fake, fake, 0), (5, 4, 1, fake, fake, 0),
                                         (4, 4097, 1, fake, fake, 0), (4, 4, -1, fake, fake, 0),
                                         (4, 4, 1, None, fake, 0), (4, 4, 1, fake, None, 0),
                                         (4, 4, 1, fake, fake, _lib.SH_FLAG_LBAP_MW | _lib.SH_FLAG_LBAP_SW),
                                         (4, 1025, 1, fake, fake, _lib.SH_FLAG_LBAP_SW)):
            assert f(C, nr, nc, B, None, col, None, flags, None) == _lib.SH_ERR_ARGS, (suf, nr, nc, B, flags)
            assert _lib.last_error()
        assert f(None, 4, 4, 0, None, None, None, 0, None) == _lib.SH_OK  # B == 0: a no-op


def test_front_ends_raise_before_any_gpu_call():
    import santa_hip
    solve, lba = santa_hip.solve_bottleneck_batched, santa_hip.linear_bottleneck_assignment
    with pytest.raises(ValueError, match="expected"):
        solve(torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="4097"):
        solve(torch.zeros((1, 2, 4097), dtype=torch.int32))
    with pytest.raises(TypeError, match="unsupported dtype"):
        solve(torch.zeros((1, 4, 4), dtype=torch.int16))
    C = torch.zeros((2, 3, 5), dtype=torch.float32)
    with pytest.raises(ValueError, match="tall"):
        solve(C, shapes=np.array([[3, 2], [1, 1]]))
    with pytest.raises(ValueError, match="outside"):
        solve(C, shapes=np.array([[3, 6], [1, 1]]))
    with pytest.raises(ValueError, match="padded wide"):
        solve(torch.zeros((2, 5, 3)), shapes=np.array([[1, 1], [1, 1]]))
    # empty batches are answered on the host
    col, value = solve(torch.zeros((0, 3, 5), dtype=torch.float16))
    assert col.shape == (0, 3) and value.shape == (0,) and value.dtype == torch.float16
    col, value = solve(torch.zeros((2, 0, 5), dtype=torch.int64))
    assert col.shape == (2, 0) and value.tolist() == [0, 0]
    with pytest.raises(ValueError, match="2-D"):
        lba(np.zeros(3))
    with pytest.raises(ValueError, match="4097"):
        lba(np.zeros((4097, 2)))
    with pytest.raises(ValueError, match="invalid numeric"):
        lba(np.array([[1.0, np.nan], [2.0, 3.0]]))
    with pytest.raises(TypeError, match="unsupported dtype"):
        lba(np.zeros((2, 2), dtype=complex))
    r, c, v = lba(np.zeros((0, 3), dtype=np.float32))
    assert r.size == 0 and c.size == 0 and v == 0 and v.dtype == np.float32


def test_lbap_kernels_have_no_scratch_and_clean_names(tmp_path):
    meta = _kernel_meta(tmp_path)
    mine = {k: v for k, v in meta.items() if "lbap" in k}
    assert len(mine) == 60, sorted(mine)  # six dtypes x (five one-wave + five multi-wave) configurations
    assert all("lbap_kernel" in k for k in mine)
    assert not {k: v for k, v in mine.items() if v}, "lbap_ kernels with private (scratch) memory"
    assert not [k for k in mine if "lsap_" in k]
