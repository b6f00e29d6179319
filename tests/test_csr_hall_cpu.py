"""CPU tests of the maximum-cardinality matching on the CSR and its Hall
certificate (lsap_match_csr_, lsap_check_hall_csr_): the host references on the
pattern families, the C ABI's argument checks (answered before any device
call) and the Python front ends' errors and empty batches on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import csr_hall_families as F
import csr_hall_ref as R
import lsap_sparse_families as S
from conftest import ROOT
from santa_hip import _lib, lsap

I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64


def _instances(module, family, nr, nc):
    """(indptr, indices, data, shape) of each instance of the case's batch."""
    b = F.batch_of(module, family, nr, nc)
    for k in range(len(b.dense)):
        ip = b.indptr[k * nr:(k + 1) * nr + 1]
        yield k, ip, b.indices, b.data, (b.corners[k] if b.corners else None), b.feasible[k]


@pytest.mark.parametrize("module,family,nr,nc", F.all_cases())
def test_references_on_the_families(module, family, nr, nc):
    for k, ip, idx, val, shape, feasible in _instances(module, family, nr, nc):
        nrb, ncb, kind = R.shape_kind(nr, nc, shape)
        card, wit = R.match_ref(ip, idx, val, nr, nc, shape)
        if kind != "live":
            assert card == 0 and not wit.any()
            continue
        if feasible is not None:
            assert (card == nrb) == bool(feasible), (k, card)
        assert not wit[nrb:].any() and (wit.any() == (card < nrb))
        # the witness does not depend on the maximum matching scipy happens to return
        rng = np.random.default_rng(k)
        E = R.edges(ip, idx, val, nr, nc, shape)
        for _ in range(3):
            order = np.concatenate([rng.permutation(nrb), np.arange(nrb, nr)])
            m = R.scipy_matching(E, order)
            assert (m >= 0).sum() == card
            assert np.array_equal(R.reachable_rows(E, m, nrb), wit), (k, "the witness moved with the matching")
            (nM, nR, nN), flags = R.check_ref(ip, idx, val, nr, nc, np.where(np.arange(nr) < nrb, m, -1), wit, shape)
            assert nM == card and nR - nN == nrb - card
            assert flags == (0 if card == nrb else R.DEFICIENT)
        if family == "chain_closed":
            assert card == nr - 1 and wit.all() and nN == nr - 1
        if family == "chain_open":
            assert card == nr


def test_inf_edges_is_feasible_for_a_presence_mask_only():
    for nr, nc in F.SHAPES:
        g = F.inf_edges(nr, nc, 1)
        assert R.match_ref(g.indptr, g.indices, None, nr, nc)[0] == nr
        assert R.match_ref(g.indptr, g.indices, g.data, nr, nc)[0] < nr
        assert np.isinf(g.data).any()


def test_last_word_rows_sit_at_the_ends_of_the_last_word():
    for nr, nc in F.SHAPES:
        g = F.last_word(nr, nc, 0)
        card, wit = R.match_ref(g.indptr, g.indices, g.data, nr, nc)
        E = R.edges(g.indptr, g.indices, g.data, nr, nc)
        lo = 64 * ((nc - 1) // 64)
        confined = [i for i in range(nr) if set(np.flatnonzero(E[i])) <= {lo, nc - 1}]
        assert len(confined) >= min(3, nr)
        if nr >= 3:
            assert card < nr and wit[confined].all()
        if nc % 64 == 0:
            assert (nc - 1) % 64 == 63 and lo % 64 == 0


def test_check_ref_flags_each_tampering():
    g = F.deficient_k(40, 129, 0)
    card, wit = R.match_ref(g.indptr, g.indices, g.data, 40, 129)
    E = R.edges(g.indptr, g.indices, g.data, 40, 129)
    m = R.scipy_matching(E)
    args = (g.indptr, g.indices, g.data, 40, 129)
    assert R.check_ref(*args, m, wit)[1] == R.DEFICIENT
    w = wit.copy()
    w[np.flatnonzero(wit)[0]] = 0
    assert R.check_ref(*args, m, w)[1] & R.WITNESS
    w = wit.copy()
    # (a row outside the witness brings its own column at least: the set stays a proof only if that is all)
    seen = E[wit != 0].any(axis=0)
    new = [(int((E[i] & ~seen).sum()), i) for i in np.flatnonzero(wit == 0)]
    for count, i in (min(new), max(new)):
        w = wit.copy()
        w[i] = 1
        assert count >= 1 and bool(R.check_ref(*args, m, w)[1] & R.WITNESS) == (count > 1)
    assert max(new)[0] > 1
    i = int(np.flatnonzero(m >= 0)[0])
    bad = m.copy()
    bad[i] = int(np.flatnonzero(~E[i])[0])
    assert R.check_ref(*args, bad, wit)[1] & R.MATCH
    bad = m.copy()
    other = int(np.flatnonzero(m >= 0)[1])
    bad[i] = m[other]
    assert R.check_ref(*args, bad, wit)[1] & R.MATCH
    assert R.check_ref(*args, m, wit, shape=(41, 129)) == ((0, 0, 0), R.MATCH)
    assert R.check_ref(*args, np.full(40, -1), np.zeros(40), shape=(0, 5)) == ((0, 0, 0), 0)


# ---------------------------------------------------------------------------
# The C ABI and the code object
# ---------------------------------------------------------------------------
def test_kernels_exist_without_scratch_and_outside_the_lsap_set(tmp_path):
    from test_kernel_resources_cpu import _kernel_meta
    meta = _kernel_meta(tmp_path)
    for name, count in (("csr_cert_kernel", 2), ("csr_slack_kernel", 2), ("csr_edges_kernel", 2), ("csr_match_kernel", 1),
                        ("csr_hall_check_kernel", 2)):
        mine = {k: v for k, v in meta.items() if name in k}
        assert len(mine) == count, (name, sorted(mine))
        assert not any("lsap_" in k for k in mine), sorted(mine)
        assert not any(mine.values()), f"{name} has private (scratch) memory: {mine}"



NEW = ("lsap_check_duals_csr", "lsap_match_csr", "lsap_check_hall_csr")


def _header_arguments(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "santa_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(arg):
    if "*" in arg:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t}[arg.split()[0]]


@pytest.mark.parametrize("name", [n + s for n in NEW for s in ("_f64", "_f32")])
def test_signatures_equal_the_header(name):
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args == [_ctype_of(a) for a in _header_arguments(name)]
    assert hasattr(_lib.lib(), name)


def test_hall_bits_equal_the_header():
    src = open(os.path.join(ROOT, "include", "santa_hip.h")).read()
    for name in ("SH_HALL_MATCH", "SH_HALL_WITNESS", "SH_HALL_DEFICIENT"):
        assert int(re.search(r"#define " + name + r" (\d+)", src).group(1)) == getattr(_lib, name)
    import santa_hip
    assert (santa_hip.SH_HALL_MATCH, santa_hip.SH_HALL_WITNESS, santa_hip.SH_HALL_DEFICIENT) == (1, 2, 4)


P = ctypes.c_void_p(64)  # a non-null, 8-byte aligned pointer that a refused call never follows


def _match(suf, nr, nc, B, indptr=P, match=P, card=P, wit=P, work=P, work_bytes=None):
    L = _lib.lib()
    if work_bytes is None:
        work_bytes = L.lsap_csr_work_bytes(nr, nc, B)
    return getattr(L, "lsap_match_csr_" + suf)(indptr, None, None, nr, nc, B, None, match, card, wit, work,
                                               work_bytes, 0, None)


def _check(suf, nr, nc, B, indptr=P, match=P, wit=P, counts=P, flags=P):
    return getattr(_lib.lib(), "lsap_check_hall_csr_" + suf)(indptr, None, None, nr, nc, B, None, match, wit, counts,
                                                             flags, None)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_argument_checks_answer_without_a_gpu(suf):
    E = _lib.SH_ERR_ARGS
    for call in (_match, _check):
        assert call(suf, 0, 4, 1) == E and call(suf, 5, 4, 1) == E and call(suf, 2, 4097, 1) == E
        assert call(suf, 2, 4, -1) == E
        assert call(suf, 2, 4, 1, indptr=None) == E and "indptr" in _lib.last_error()
        assert call(suf, 2, 4, 1, match=None) == E and call(suf, 2, 4, 1, wit=None) == E
        # B == 0 is a no-op after the checks, whatever the pointers
        assert call(suf, 2, 4, 0, indptr=None, match=None, wit=None) == _lib.SH_OK
        assert call(suf, 0, 4, 0) == E
    assert _match(suf, 2, 4, 1, card=None) == E
    assert _match(suf, 2, 4, 1, work=None) == E
    assert _match(suf, 2, 4, 1, work_bytes=8) == E and "lsap_csr_work_bytes" in _lib.last_error()
    assert _match(suf, 2, 4, 1, work=ctypes.c_void_p(68)) == E
    assert _match(suf, 2, 4, 0, card=None, work=None, work_bytes=0) == _lib.SH_OK
    assert _check(suf, 2, 4, 1, counts=None) == E and _check(suf, 2, 4, 1, flags=None) == E


# ---------------------------------------------------------------------------
# The Python front ends, on CPU tensors: every answer here precedes the GPU
# ---------------------------------------------------------------------------
def _raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and text in str(e.value), str(e.value)


def _full(shape, dtype=F64):
    B, NR, NC = shape
    return (torch.arange(B * NR + 1, dtype=I64) * NC, torch.arange(NC, dtype=I32).repeat(B * NR),
            torch.ones(B * NR * NC, dtype=dtype))


def test_front_end_errors():
    crow, idx, val = _full((2, 3, 4))
    mm, cm = lsap.maximum_matching_sparse, lsap.check_matching_sparse
    match, wit = torch.zeros((2, 3), dtype=I32), torch.zeros((2, 3), dtype=torch.uint8)
    _raises(ValueError, "shape = (B, NR, NC) is required", lambda: mm(crow, idx, val))
    _raises(ValueError, "shape = (B, NR, NC) is required", lambda: cm(crow, idx, val, (3, 4), match, wit))
    _raises(ValueError, "a sparse batch must be wide, got [4, 3]", lambda: mm(crow, idx, val, shape=(2, 4, 3)))
    _raises(ValueError, "max(NR, NC) = 4097 > 4096", lambda: mm(crow, idx, None, shape=(1, 2, 4097)))
    _raises(ValueError, "max(NR, NC) = 4097 > 4096", lambda: cm(crow, idx, None, (1, 2, 4097), match, wit))
    _raises(TypeError, "unsupported dtype torch.complex64", lambda: mm(crow, idx, val.to(torch.complex64), shape=(2, 3, 4)))
    _raises(ValueError, "crow must have B * NR + 1 = 7 entries", lambda: mm(crow[:-1], idx, val, shape=(2, 3, 4)))
    _raises(ValueError, "crow must have B * NR + 1 = 7 entries", lambda: mm(crow[:-1], idx, None, shape=(2, 3, 4)))
    _raises(ValueError, "crow must have B * NR + 1 entries", lambda: mm(crow[:-1], idx, None, shape=(2, 3, 4), validate=False))
    bad = idx.clone()
    bad[1] = 7
    _raises(ValueError, "a column index lies outside [0, 4)", lambda: mm(crow, bad, None, shape=(2, 3, 4)))
    _raises(ValueError, "shapes[1] = (4, 4) is outside the padded [3, 4] matrix",
            lambda: mm(crow, idx, val, shape=(2, 3, 4), shapes=[[3, 4], [4, 4]]))
    # with maximize the forbidden value is -inf; +inf is then no number
    inf = val.clone()
    inf[0] = float("inf")
    _raises(ValueError, "invalid numeric entries", lambda: mm(crow, idx, inf, shape=(2, 3, 4), maximize=True))
    _raises(ValueError, "invalid numeric entries", lambda: mm(crow, idx, -inf, shape=(2, 3, 4)))
    _raises(ValueError, "expected match and wit of shape [2, 3]", lambda: cm(crow, idx, val, (2, 3, 4), match[:, :2], wit))
    _raises(ValueError, "expected match and wit of shape [2, 3]", lambda: cm(crow, idx, val, (2, 3, 4), match, wit[:1]))
    _raises(TypeError, "wit must be uint8 or bool", lambda: cm(crow, idx, val, (2, 3, 4), match, wit.int()))
    _raises(TypeError, "col must be an integer tensor", lambda: cm(crow, idx, val, (2, 3, 4), match.float(), wit))
    _raises(ValueError, "max(nr, nc) = 4097 > 4096",
            lambda: lsap.maximum_bipartite_matching((np.zeros(4098, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                                     np.zeros(0), (4097, 2))))


@pytest.mark.parametrize("shape", [(0, 3, 4), (2, 0, 4), (2, 0, 0)], ids=str)
def test_empty_batches(shape):
    B, NR, NC = shape
    crow, none_i, none_v = torch.zeros(B * NR + 1, dtype=I64), torch.zeros(0, dtype=I32), torch.zeros(0, dtype=F32)
    for val in (none_v, None):
        match, card, wit = lsap.maximum_matching_sparse(crow, none_i, val, shape=shape)
        assert tuple(match.shape) == (B, NR) and match.dtype == I32 and bool((match == -1).all())
        assert tuple(card.shape) == (B,) and card.dtype == I32 and not card.any()
        assert tuple(wit.shape) == (B, NR) and wit.dtype == torch.uint8 and not wit.any()
        counts, flags = lsap.check_matching_sparse(crow, none_i, val, shape, match, wit)
        assert tuple(counts.shape) == (B, 3) and counts.dtype == I32 and not counts.any()
        assert tuple(flags.shape) == (B,) and flags.dtype == I32 and not flags.any()
    assert all(t.device.type == "cpu" for t in (match, card, wit, counts, flags))


def test_maximum_bipartite_matching_of_an_empty_matrix():
    for nr, nc in ((0, 0), (0, 3), (3, 0)):
        m = lsap.maximum_bipartite_matching((np.zeros(nr + 1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                             np.zeros(0), (nr, nc)))
        assert m.dtype == np.int64 and m.shape == (nr,) and (m == -1).all()
