"""The bottleneck solver's witness and certificate without a GPU: the two host
references against each other and against lbap_ref, the mutations and families
that the GPU tests use pinned on the references alone, the library surface and
the new kernels' metadata."""
import os
import re

import numpy as np
import pytest
import torch

import lbap_cert_families as F
from conftest import ROOT
from lbap_cert_ref import (SH_LBCERT_COL, SH_LBCERT_NONE, SH_LBCERT_VALUE, SH_LBCERT_WITNESS, lbap_check_ref,
                           lbap_witness_ref)
from lbap_ref import lbap_ref
from santa_hip import _lib
from test_kernel_resources_cpu import _kernel_meta

SUFFIXES = ("i64", "i32", "f64", "f32", "f16", "bf16")
I64 = np.iinfo(np.int64)


def _instances():
    """(C, maximize): 360 seeded instances of at most 12 rows."""
    rng = np.random.default_rng(2025)
    for t in range(360):
        nr = int(rng.integers(1, 13))
        nc = int(rng.integers(nr, 17))
        kind, maximize = t % 6, bool(t & 8)
        if kind == 0:
            yield rng.integers(0, 4, size=(nr, nc)).astype(np.int64), maximize           # ties
        elif kind == 1:
            yield rng.integers(I64.min, I64.max, size=(nr, nc), endpoint=True), maximize  # the whole int64 range
        elif kind == 2:
            C = rng.integers(-3, 4, size=(nr, nc)).astype(np.int64)
            C[rng.random((nr, nc)) < 0.2] = I64.min
            C[rng.random((nr, nc)) < 0.2] = I64.max
            yield C, maximize
        elif kind == 3:
            C = rng.integers(0, 4, size=(nr, nc)).astype(np.float32)
            C[rng.random((nr, nc)) < 0.75] = -np.inf if maximize else np.inf          # often infeasible
            C[rng.random((nr, nc)) < 0.05] = np.inf if maximize else -np.inf          # the best cost
            yield C, maximize
        elif kind == 4:
            C = rng.integers(-1, 2, size=(nr, nc)).astype(np.float64)
            C[rng.random((nr, nc)) < 0.3] = np.nan
            C[C == 0] = -0.0                                                            # signed zeros
            C[rng.random((nr, nc)) < 0.3] *= -1
            yield C, maximize
        else:
            yield rng.integers(-50, 50, size=(nr, nc)).astype(np.int32), maximize


def test_witness_reference_keeps_the_solution_and_the_certificate_accepts_it():
    n = infeasible = 0
    for C, maximize in _instances():
        col, value, wit = lbap_witness_ref(C, maximize)
        rcol, rvalue, _, _ = lbap_ref(C, maximize)
        assert np.array_equal(col, rcol) and value == rvalue and type(value) is type(rvalue), (C, maximize)
        nR, nN, flags = lbap_check_ref(C, col, value, wit, maximize)
        n += 1
        if (col < 0).any():
            infeasible += 1
            assert flags == SH_LBCERT_NONE, (C, maximize, flags)
        else:
            assert flags == 0, (C, maximize, flags)
        assert nN == nR - 1 and nR == int(wit.sum()) >= 1, (C, maximize, nR, nN)
    assert n >= 300 and 10 <= infeasible <= n // 3


def test_each_mutation_raises_its_bit():
    cases = F.mutation_cases()
    assert len(cases) >= 2 * (1 + 14 + 1 + 1 + 2)
    for name, C, col, value, wit, maximize, bit in cases:
        _, _, flags = lbap_check_ref(C, col, value, wit, maximize)
        assert flags & bit, (name, flags)
        if bit == F.WITNESS and "worse" in name:  # a valid assignment and its true value: nothing else is wrong
            assert flags == SH_LBCERT_WITNESS, (name, flags)
        if "infeasible" in name:
            assert flags == SH_LBCERT_WITNESS | SH_LBCERT_NONE, (name, flags)
    # an integer instance has no infeasible answer, and a malformed one is flagged, not followed
    C = np.arange(12, dtype=np.int64).reshape(3, 4)
    none = np.full(3, -1)
    assert lbap_check_ref(C, none, 0, np.ones(3, np.uint8))[2] & (SH_LBCERT_COL | SH_LBCERT_NONE) == 9
    assert lbap_check_ref(C, [0, 99, -7], 0, np.ones(3, np.uint8))[2] & SH_LBCERT_COL
    assert lbap_check_ref(C, [0, 1, -1], 5, np.ones(3, np.uint8))[2] & SH_LBCERT_COL
    assert lbap_check_ref(C, [0, 1, 2], 9, np.ones(3, np.uint8))[2] & SH_LBCERT_VALUE
    assert lbap_check_ref(np.zeros((2, 3)), [0, 1], -0.0, [1, 0])[2] == 0  # -0.0 equals +0.0
    assert lbap_check_ref(np.zeros((4, 4), np.int32), [-1] * 4, 0, [0] * 4, shape=(0, 3)) == (0, 0, 0)
    assert lbap_check_ref(np.zeros((4, 4), np.int32), [0, -1, -1, -1], 0, [0] * 4, shape=(0, 3))[2] == SH_LBCERT_COL
    assert lbap_check_ref(np.zeros((4, 4), np.int32), [0, 1, 5, -1], 0, [1, 0, 9, 9], shape=(2, 3)) == \
        (1, 0, SH_LBCERT_COL)


SIZES = ((2, 2), (3, 7), (7, 7), (33, 40), (65, 65))


@pytest.mark.parametrize("family", ["rise_every_search", "whole_rows", "early_rise", "tie_no_rewrite"])
def test_closed_forms_are_the_reference(family):
    for nr, nc in SIZES:
        C = F.build(family, nr, nc)
        rises = []
        col, value, wit = lbap_witness_ref(C, rise=lambda mv, top: rises.append(mv > top) or mv > top)
        want = F.closed_form(family, nr, nc)
        assert np.array_equal(col, want[0]) and value == want[1] and np.array_equal(wit, want[2]), (family, nr, nc)
        nR, nN, flags = lbap_check_ref(C, col, value, wit)
        assert flags == 0 and nN == nR - 1
        if family == "rise_every_search":
            assert sum(rises) == nr - 1 and (nR, nN) == (1, 0)        # every search after the first rises
        elif family == "whole_rows":
            assert sum(rises) == (1 if nr > 1 else 0) and rises[-1] and nR == nr  # the last search, and only it
        else:
            assert not any(rises) and nR == 1
        if family == "tie_no_rewrite":   # the rule `>=` rewrites the witness at the tie
            other = lbap_witness_ref(C, rise=lambda mv, top: mv >= top)[2]
            assert other.sum() == nr and not np.array_equal(other, wit)
            assert lbap_check_ref(C, col, value, other)[2] == 0  # (a proof as well, but not the normative one)
        if family == "early_rise":       # the last search visited every other row without rising
            assert lbap_ref(C)[2] == nr - 1 or nr == 2


def test_infeasible_hall_is_pinned():
    for nr, nc, k in ((2, 2, 1), (7, 9, 3), (33, 40, 11), (65, 65, 64)):
        C = F.infeasible_hall(nr, nc, k)
        col, value, wit = lbap_witness_ref(C)
        want = F.closed_form("infeasible_hall", nr, nc, k)
        assert np.array_equal(col, want[0]) and value == want[1] and np.array_equal(wit, want[2])
        assert lbap_check_ref(C, col, value, wit) == (k + 1, k, SH_LBCERT_NONE)
        # one finite entry more for the last row and the instance is feasible
        C[nr - 1, nc - 1] = 7
        assert (lbap_witness_ref(C)[0] >= 0).all()


def test_maximize_full_range_needs_all_64_bits():
    for nr, nc, k in ((9, 12, 0), (40, 60, 1)):
        C = F.maximize_full_range(nr, nc, k)
        assert (C == I64.min).any() and (C == I64.max).any()
        col, value, wit = lbap_witness_ref(C, True)
        assert np.array_equal(col, lbap_ref(C, True)[0])
        nR, nN, flags = lbap_check_ref(C, col, value, wit, True)
        assert flags == 0 and nN == nR - 1
        # keys compared as signed, or by their high word alone, accept a wrong value or refuse the right one
        assert lbap_check_ref(C, col, value, wit, False)[2] != 0


def test_cases_reach_every_witness_kernel():
    want = {(nw, k, dt) for dt in F.DTYPES for nw, k in
            ((1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (4, 1), (4, 2), (4, 4), (8, 4), (16, 4))}
    assert F.configs_reached() == want
    for dt in F.DTYPES:   # every closed form is exact in the dtype it runs in
        for n in F.SEAM_SIZES[dt] + (F.SW_SEAM,):
            for family, k in F.seam_members(dt, n):
                assert F.fits(family, dt, n)
        V = np.array([0, 1, 2, 5, F.BIG])
        assert np.array_equal(F.widen(F.store(V, dt), dt), V)


# --------------------------------------------------------------------------- the library
def _params(header, name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header)
    assert m, f"{name} is not declared in santa_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_library_exports_the_entries_with_the_header_signatures():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "santa_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for suf in SUFFIXES:
        for name, n in (("lbap_solve_wit_" + suf, 10), ("lbap_check_" + suf, 12)):
            assert hasattr(L, name), name
            res, args = _lib.SIGNATURES[name]
            params = _params(header, name)
            assert res is _lib._I and len(params) == len(args) == n
            for p, a in zip(params, args):
                want = _lib._P if "*" in p else _lib._U if p.startswith("unsigned") else _lib._I
                assert a is want, (name, p, a)
        # lbap_solve_ is what it was, and the witness entry is it with uint8_t *d_wit before the flags
        solve, wit = _params(header, "lbap_solve_" + suf), _params(header, "lbap_solve_wit_" + suf)
        assert len(solve) == 9 and wit[:7] == solve[:7] and wit[8:] == solve[7:] and wit[7] == "uint8_t *d_wit"
    for flag, bit in (("SH_LBCERT_COL", 1), ("SH_LBCERT_VALUE", 2), ("SH_LBCERT_WITNESS", 4), ("SH_LBCERT_NONE", 8)):
        assert getattr(_lib, flag) == bit == globals()[flag]
        assert re.search(r"#define %s %d\b" % (flag, bit), header)


def test_c_abi_checks_its_arguments_before_any_device_call():
    """Every refusal is SH_ERR_ARGS with a text; none of them needs a GPU."""
    L = _lib.lib()
    fake = 4096  # a non-null pointer that is never dereferenced
    bad = ((0, 4, 1, fake, fake, 0), (5, 4, 1, fake, fake, 0), (4, 4097, 1, fake, fake, 0), (4, 4, -1, fake, fake, 0),
           (4, 4, 1, None, fake, 0), (4, 4, 1, fake, None, 0),
           (4, 4, 1, fake, fake, _lib.SH_FLAG_LBAP_MW | _lib.SH_FLAG_LBAP_SW), (4, 1025, 1, fake, fake, _lib.SH_FLAG_LBAP_SW))
    for suf in SUFFIXES:
        solve, check = getattr(L, "lbap_solve_wit_" + suf), getattr(L, "lbap_check_" + suf)
        for nr, nc, B, C, col, flags in bad:   # lbap_solve_'s refusals, in both
            assert solve(C, nr, nc, B, None, col, None, fake, flags, None) == _lib.SH_ERR_ARGS, (suf, nr, nc, B, flags)
            assert _lib.last_error()
            assert check(C, nr, nc, B, None, col, fake, fake, fake, fake, flags, None) == _lib.SH_ERR_ARGS
            assert _lib.last_error()
        assert solve(fake, 4, 4, 1, None, fake, None, None, 0, None) == _lib.SH_ERR_ARGS  # wit is required
        assert "wit" in _lib.last_error()
        for miss in range(4):  # value, wit, counts, flags
            ptrs = [None if q == miss else fake for q in range(4)]
            assert check(fake, 4, 4, 1, None, fake, *ptrs, 0, None) == _lib.SH_ERR_ARGS, (suf, miss)
        assert solve(None, 4, 4, 0, None, None, None, None, 0, None) == _lib.SH_OK  # B == 0: a no-op
        assert check(None, 4, 4, 0, None, None, None, None, None, None, 0, None) == _lib.SH_OK


def test_front_ends_raise_and_answer_empty_batches_without_a_gpu():
    import santa_hip
    solve, check, lba = (santa_hip.solve_bottleneck_batched, santa_hip.check_bottleneck,
                         santa_hip.linear_bottleneck_assignment)
    z = torch.zeros
    for call in (lambda C, **kw: solve(C, witness=True, **kw),
                 lambda C, **kw: check(C, z(C.shape[:2] if C.dim() == 3 else 1, dtype=torch.int32), z(C.shape[0]),
                                       z(C.shape[0], 1, dtype=torch.uint8), **kw)):
        with pytest.raises(ValueError, match="expected"):
            call(z((4, 4), dtype=torch.int64))
        with pytest.raises(ValueError, match="4097"):
            call(z((1, 2, 4097), dtype=torch.int32))
        with pytest.raises(TypeError, match="unsupported dtype"):
            call(z((1, 4, 4), dtype=torch.int16))
        with pytest.raises(ValueError, match="tall"):
            call(z((2, 3, 5)), shapes=np.array([[3, 2], [1, 1]]))
        with pytest.raises(ValueError, match="outside"):
            call(z((2, 3, 5)), shapes=np.array([[3, 6], [1, 1]]))
        with pytest.raises(ValueError, match="padded wide"):
            call(z((2, 5, 3)), shapes=np.array([[1, 1], [1, 1]]))
    C = z((2, 3, 5))
    with pytest.raises(ValueError, match="expected col"):
        check(C, z((2, 3), dtype=torch.int32), z(2), z((2, 5), dtype=torch.uint8))
    with pytest.raises(TypeError, match="value must be"):
        check(C, z((2, 3), dtype=torch.int32), z(2, dtype=torch.float64), z((2, 3), dtype=torch.uint8))
    # empty batches are answered on the host; wit is over the shorter side
    col, value, wit = solve(z((0, 3, 5), dtype=torch.float16), witness=True)
    assert col.shape == (0, 3) and value.shape == (0,) and wit.shape == (0, 3) and wit.dtype == torch.uint8
    col, value, wit = solve(z((2, 0, 5), dtype=torch.int64), witness=True)
    assert col.shape == (2, 0) and value.tolist() == [0, 0] and wit.shape == (2, 0)
    col, value, wit = solve(z((2, 5, 0), dtype=torch.int64), witness=True)
    assert col.shape == (2, 5) and (col == -1).all() and wit.shape == (2, 0)
    assert len(solve(z((0, 3, 5)))) == 2  # without the keyword: what it always returned
    for shape in ((0, 3, 5), (2, 0, 5), (2, 5, 0)):
        B, NR, NC = shape
        nR, nN, flags = check(z(shape), torch.full((B, NR), -1, dtype=torch.int32), z(B),
                              z((B, min(NR, NC)), dtype=torch.uint8))
        assert nR.shape == nN.shape == flags.shape == (B,) and not flags.any() and not nR.any() and not nN.any()
        assert flags.dtype == nR.dtype == torch.int32
    r, c, v, w = lba(np.zeros((0, 3), dtype=np.float32), witness=True)
    assert r.size == 0 and c.size == 0 and v == 0 and w.shape == (0,) and w.dtype == bool
    with pytest.raises(ValueError, match="invalid numeric"):
        lba(np.array([[1.0, np.nan], [2.0, 3.0]]), witness=True)


def test_witness_and_check_kernels_have_no_scratch_and_clean_names(tmp_path):
    meta = _kernel_meta(tmp_path)
    wit = {k: v for k, v in meta.items() if "bneck_wit_kernel" in k}
    chk = {k: v for k, v in meta.items() if "bneck_check_kernel" in k}
    assert len(wit) == 60, sorted(wit)  # six dtypes x (five one-wave + five multi-wave) configurations
    assert len(chk) == 6, sorted(chk)
    assert not {k: v for k, v in {**wit, **chk}.items() if v}, "kernels with private (scratch) memory"
    assert not [k for k in {**wit, **chk} if "lbap" in k or "lsap_" in k]
