"""Floating-point dtypes of the batched LSAP on the CPU (no GPU calls).

* the float32 / float16 / bfloat16 entries are declared in the header, bound
  in _lib.SIGNATURES and exported by the library;
* they give the f64 entry's host-side refusals before any device call;
* SH_FLAG_F64_MW and SH_FLAG_F64_SW together are refused on all four float
  entries;
* solve_batched still refuses dtypes outside its list.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from santa_hip import _lib, lsap
from test_cabi_cpu import declared_functions

NARROW = ("lsap_solve_batched_rect_f32", "lsap_solve_batched_rect_f16", "lsap_solve_batched_rect_bf16")
FLOAT = ("lsap_solve_batched_rect_f64",) + NARROW


def test_float_entries_declared_bound_and_exported():
    names = declared_functions()
    L = _lib.lib()
    for name in NARROW:
        assert name in names and name in _lib.SIGNATURES and hasattr(L, name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["lsap_solve_batched_rect_f64"]
    assert set(lsap.FLOAT_ENTRIES.values()) == set(FLOAT)


def _rect(name, nr, nc, B, C=1, col=1, flags=1):
    """Call a float entry with dummy non-null pointers (never dereferenced:
    every case here is answered by the host-side checks)."""
    p = lambda x: ctypes.c_void_p(0x1000) if x else None  # noqa: E731
    return getattr(_lib.lib(), name)(p(C), nr, nc, B, None, p(col), None, flags, None)


@pytest.mark.parametrize("name", NARROW)
def test_float_host_checks_without_gpu(name):
    E = _lib.SH_ERR_ARGS
    assert _rect(name, 0, 5, 1) == E           # nr < 1
    assert _rect(name, -1, 5, 1) == E
    assert _rect(name, 6, 5, 1) == E           # nr > nc: tall is the caller's transpose
    assert "transpose" in _lib.last_error()
    assert _rect(name, 5, _lib.SH_MAX_N + 1, 1) == E
    assert _rect(name, 3, 5, -1) == E          # B < 0
    assert _rect(name, 3, 5, 1, col=0) == E    # null col
    assert _rect(name, 3, 5, 1, C=0) == E      # null C
    assert _rect(name, 3, 5, 0) == _lib.SH_OK  # B == 0: a no-op
    assert _rect(name, 3, 5, 0, C=0, col=0) == _lib.SH_OK
    assert _rect(name, 1024, 1024, 0) == _lib.SH_OK


@pytest.mark.parametrize("name", FLOAT)
def test_both_design_flags_are_refused(name):
    both = _lib.SH_FLAG_F64_MW | _lib.SH_FLAG_F64_SW
    assert (_lib.SH_FLAG_F64_MW, _lib.SH_FLAG_F64_SW) == (16384, 32768)
    for nr, nc in ((3, 5), (100, 300)):
        assert _rect(name, nr, nc, 1, flags=1 | both) == _lib.SH_ERR_ARGS
        assert "exclude" in _lib.last_error()
    # either flag alone passes the host checks (B == 0: nothing is launched)
    assert _rect(name, 100, 300, 0, flags=1 | _lib.SH_FLAG_F64_MW) == _lib.SH_OK
    assert _rect(name, 100, 300, 0, flags=1 | _lib.SH_FLAG_F64_SW) == _lib.SH_OK


def test_header_defines_the_design_flags():
    src = open(os.path.join(ROOT, "include", "santa_hip.h")).read()
    assert re.search(r"#define SH_FLAG_F64_MW 16384u\b", src)
    assert re.search(r"#define SH_FLAG_F64_SW 32768u\b", src)


@pytest.mark.parametrize("dt", [torch.int16, torch.complex64])
def test_solve_batched_refuses_other_dtypes(monkeypatch, dt):
    monkeypatch.setattr(lsap, "require_gpu", lambda: None)
    with pytest.raises(TypeError, match="unsupported dtype"):
        lsap.solve_batched(torch.zeros((2, 3, 4), dtype=dt))
