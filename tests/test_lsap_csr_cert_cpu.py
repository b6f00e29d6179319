"""CPU tests of the min-sum certificate on the CSR (lsap_check_duals_csr_):
the host reference on the sparse families with the duals of the replay of
scipy's run, the rules of the header on hand-made instances, the C ABI's
argument checks (answered before any device call) and check_duals_sparse's
errors and empty batches on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import lsap_cert_ref as C
import lsap_sparse_families as S
from lsap_csr_cert_ref import csr_cert_ref, densify_one
from santa_hip import _lib, lsap

I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
CASES = [(f, nr, nc) for f, nr, nc in S.cases() if nr <= 100 and nc <= 1025]


@pytest.mark.parametrize("family,nr,nc", CASES)
def test_replayed_duals_certify_every_feasible_instance(family, nr, nc):
    b = S.batch(family, nr, nc)
    col, u, v = S.expected(family, nr, nc)
    for k in range(len(b.dense)):
        ip = b.indptr[k * nr:(k + 1) * nr + 1]
        shape = b.corners[k] if b.corners else None
        slack, flags = csr_cert_ref(ip, b.indices, b.data, nr, nc, col[k], u[k], v[k], shape)
        live = b.dense[k].shape[0] > 0
        assert flags == (0 if b.feasible[k] or not live else C.NONE), (k, flags, slack)
        if b.feasible[k]:
            assert slack[0] >= 0 and slack[1] == 0
        # the definition: the dense reference on the densification
        want = C.cert_ref(densify_one(ip, b.indices, b.data, nr, nc), col[k], u[k], v[k], shape)
        assert C.same_bits(slack, np.array(want[:3], dtype=np.float64)) and flags == want[3]


def _csr(D):
    P = np.isfinite(D) | np.isnan(D)
    return S.csr_of(P, np.where(P, D, 0))


def test_rules_of_the_header_on_a_small_instance():
    inf = np.inf
    D = np.array([[1.0, inf, 4.0], [inf, 2.0, inf]])
    ip, idx, val = _csr(D)
    col, u, v = np.array([0, 1]), np.array([1.0, 2.0]), np.zeros(3)
    slack, flags = csr_cert_ref(ip, idx, val, 2, 3, col, u, v)
    assert flags == 0 and slack.tolist() == [0.0, 0.0, 0.0]
    # every entry stored: the minimum has no +inf to meet
    ipf, idxf, valf = S.csr_of(np.ones((2, 3), dtype=bool), np.array([[1.0, 9.0, 4.0], [9.0, 2.0, 9.0]]))
    assert csr_cert_ref(ipf, idxf, valf, 2, 3, col, u - 5, v)[0][0] == 5.0
    # a chosen pair that is not stored: matched slack +inf, TIGHT
    slack, flags = csr_cert_ref(ip, idx, val, 2, 3, np.array([1, 0]), u, v)
    assert flags == C.TIGHT and slack[1] == inf and slack[2] == -inf
    # a live dual that is not finite: slack[0] NaN and SLACK, the rest by the formulas
    for bad_u, bad_v in ((np.array([1.0, inf]), v), (u, np.array([0.0, -inf, 0.0])), (np.array([np.nan, 2.0]), v)):
        slack, flags = csr_cert_ref(ip, idx, val, 2, 3, col, bad_u, bad_v)
        assert np.isnan(slack[0]) and flags & C.SLACK
    # ... but not outside the live corner, not for NONE and not for a shape outside the matrix
    slack, flags = csr_cert_ref(ip, idx, val, 2, 3, np.array([0, -1]), np.array([1.0, inf]), v, shape=(1, 3))
    assert flags == 0 and slack[0] == 0.0
    assert csr_cert_ref(ip, idx, val, 2, 3, np.array([-1, -1]), np.array([1.0, inf]), v)[1] == C.NONE
    slack, flags = csr_cert_ref(ip, idx, val, 2, 3, col, np.array([1.0, inf]), v, shape=(3, 3))
    assert flags == C.COL and slack.tolist() == [0.0, 0.0, 0.0]
    # a stored +inf is a missing entry, a stored 0.0 an entry
    ip0, idx0, val0 = S.csr_of(np.array([[True, True]]), np.array([[inf, 0.0]]))
    assert csr_cert_ref(ip0, idx0, val0, 1, 2, np.array([1]), np.array([0.0]), np.zeros(2))[1] == 0
    assert csr_cert_ref(ip0, idx0, val0, 1, 2, np.array([0]), np.array([0.0]), np.zeros(2))[1] == C.TIGHT


# ---------------------------------------------------------------------------
P = ctypes.c_void_p(64)  # a non-null pointer that a refused call never follows


def _call(suf, nr, nc, B, indptr=P, col=P, u=P, v=P, slack=P, flags=P):
    return getattr(_lib.lib(), "lsap_check_duals_csr_" + suf)(indptr, None, None, nr, nc, B, None, col, u, v, slack,
                                                              flags, None)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_argument_checks_answer_without_a_gpu(suf):
    E = _lib.SH_ERR_ARGS
    assert _call(suf, 0, 4, 1) == E and _call(suf, 5, 4, 1) == E and _call(suf, 2, 4097, 1) == E
    assert _call(suf, 2, 4, -1) == E
    assert _call(suf, 2, 4, 1, indptr=None) == E and "indptr" in _lib.last_error()
    for name in ("col", "u", "v", "slack", "flags"):
        assert _call(suf, 2, 4, 1, **{name: None}) == E, name
    assert _call(suf, 2, 4, 0, indptr=None, col=None, u=None, v=None, slack=None, flags=None) == _lib.SH_OK
    assert _call(suf, 0, 4, 0) == E


def _raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and text in str(e.value), str(e.value)


def test_front_end_errors():
    B, NR, NC = 2, 3, 4
    crow = torch.arange(B * NR + 1, dtype=I64) * NC
    idx, val = torch.arange(NC, dtype=I32).repeat(B * NR), torch.ones(B * NR * NC, dtype=F64)
    col, u, v = torch.zeros((B, NR), dtype=I32), torch.zeros((B, NR), dtype=F64), torch.zeros((B, NC), dtype=F64)
    f = lsap.check_duals_sparse
    _raises(ValueError, "shape = (B, NR, NC) is required", lambda: f(crow, idx, val, (NR, NC), col, u, v))
    _raises(ValueError, "a sparse batch must be wide, got [4, 3]", lambda: f(crow, idx, val, (2, 4, 3), col, u, v))
    _raises(ValueError, "max(NR, NC) = 4097 > 4096", lambda: f(crow, idx, val, (1, 2, 4097), col, u, v))
    _raises(TypeError, "unsupported dtype torch.complex64", lambda: f(crow, idx, val.to(torch.complex64), (B, NR, NC), col, u, v))
    _raises(ValueError, "crow[-1] = 24 != nnz = 23", lambda: f(crow, idx[:-1], val[:-1], (B, NR, NC), col, u, v))
    _raises(ValueError, "equal lengths", lambda: f(crow, idx, val[:-1], (B, NR, NC), col, u, v, validate=False))
    _raises(ValueError, "expected col and u of shape [2, 3] and v of shape [2, 4]",
            lambda: f(crow, idx, val, (B, NR, NC), col, u, v[:, :3]))
    _raises(TypeError, "the duals of torch.float64 costs are torch.float64",
            lambda: f(crow, idx, val, (B, NR, NC), col, u.float(), v))
    _raises(TypeError, "the duals of torch.float32 costs are torch.float64",
            lambda: f(crow, idx, val.float(), (B, NR, NC), col, u, v.float()))
    _raises(TypeError, "col must be an integer tensor", lambda: f(crow, idx, val, (B, NR, NC), col.float(), u, v))
    _raises(ValueError, "shapes[1] = (3, 2) is tall", lambda: f(crow, idx, val, (B, NR, NC), col, u, v,
                                                                 shapes=[[3, 4], [3, 2]]))


@pytest.mark.parametrize("shape", [(0, 3, 4), (2, 0, 4), (2, 0, 0)], ids=str)
def test_empty_batches(shape):
    B, NR, NC = shape
    crow = torch.zeros(B * NR + 1, dtype=I64)
    col, u, v = torch.zeros((B, NR), dtype=I64), torch.zeros((B, NR), dtype=F64), torch.zeros((B, NC), dtype=F64)
    for dtype in (F32, I32):
        slack, flags = lsap.check_duals_sparse(crow, torch.zeros(0, dtype=I32), torch.zeros(0, dtype=dtype), shape,
                                               col, u, v, maximize=True)
        assert tuple(slack.shape) == (B, 3) and slack.dtype == F64 and not slack.any()
        assert tuple(flags.shape) == (B,) and flags.dtype == I32 and not flags.any()
        assert slack.device.type == "cpu" and flags.device.type == "cpu"
