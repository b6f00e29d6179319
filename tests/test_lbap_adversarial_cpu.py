"""The bottleneck solver's adversarial families on the CPU (no GPU calls): the
conditions that make the GPU tests of test_lbap_adversarial_gpu.py mean
something, asserted on the host references alone.

* `chain`: a search of exactly nr steps and a path of exactly nr hops;
* `signed_zeros`, `nan_patterns`, `split_words`: each returns another `col`
  under the wrong key it is built to catch;
* `random_bits`: feasible, with a NaN, a subnormal and a negative value;
* every live reference equals the independent threshold search, every value is
  exact in the dtype it runs in, the recorded Machol-Wien answers are optimal
  matchings, and the cases that compare `col` reach all 60 lbap_kernels.
"""
import os

import numpy as np
import pytest

import lbap_families as F
import test_lbap_adversarial_gpu as G
from conftest import ROOT
from lbap_ref import lbap_ref, threshold_value
from santa_hip import _lib
from test_lbap_gpu import designs

SMALL = [(40, 60), (65, 65), (200, 257)]


def cases_of(family):
    return [c for c in G.CASES if c.family == family]


def differs(a, b):
    return not np.array_equal(a, b)


# --------------------------------------------------------------------------- the launch table
def test_config_of_is_the_launch_table():
    """The seams that the static_asserts of santa_api.inc name, both designs,
    and the default's switch at 256 / 512 columns and 1024 instances."""
    sw, mw = F.SH_FLAG_LBAP_SW, F.SH_FLAG_LBAP_MW
    assert (sw, mw) == (_lib.SH_FLAG_LBAP_SW, _lib.SH_FLAG_LBAP_MW)
    one = {1: 1, 64: 1, 65: 2, 128: 2, 129: 4, 256: 4, 257: 8, 512: 8, 513: 16, 1024: 16}
    for nc, k in one.items():
        assert F.config_of(nc, 4, sw) == (1, k), nc
    many = {1: (4, 1), 256: (4, 1), 257: (4, 2), 512: (4, 2), 513: (4, 4), 1024: (4, 4), 1025: (8, 4),
            2048: (8, 4), 2049: (16, 4), 4096: (16, 4)}
    for nc, cfg in many.items():
        assert F.config_of(nc, 4, mw) == cfg, nc
        if nc > 1024:
            assert F.config_of(nc, 4, 0) == F.config_of(nc, 70000, 0) == cfg
    for nc, B, cfg in ((256, 1, (1, 4)), (257, 1024, (4, 2)), (257, 1025, (1, 8)), (512, 1024, (4, 2)),
                       (512, 1025, (1, 8)), (513, 70000, (4, 4)), (8, 70000, (1, 1))):
        assert F.config_of(nc, B, 0) == cfg, (nc, B)
    # the table's own text (a changed seam must move the cases with it)
    src = open(os.path.join(ROOT, "mpi-hungarian-method_amd", "csrc", "santa_api.inc")).read()
    for line in ("bool lbap_mw_default(int nc, int B) { return nc > 512 || (nc > 256 && B <= 1024); }",
                 "if (n <= 256) return go(BigCfg<4, 1, 0>{});", "if (n <= 512) return go(BigCfg<4, 2, 0>{});",
                 "if (n <= 1024) return go(BigCfg<4, 4, 0>{});", "if (n <= 2048) return go(BigCfg<8, 4, 0>{});",
                 "return go(BigCfg<16, 4, 0>{});"):
        assert line in src, line


def test_the_cases_compare_col_in_all_60_kernels():
    """Every case of the GPU module compares col with lbap_ref (live or
    recorded) in every design at its width; none of their matrices is
    constant.  Six dtypes x (five one-wave + five multi-wave) configurations."""
    have = set()
    for c in G.CASES:
        M = F.members(*c)
        assert all(np.unique(F.as_bits(S, c.dt)).size > 1 for S in M), c
        have |= {F.config_of(c.nc, len(M), flags) + (c.dt,) for _, flags in designs(c.nc)}
    want = {(nw, k, dt) for dt in F.DTYPES
            for nw, k in ((1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (4, 1), (4, 2), (4, 4), (8, 4), (16, 4))}
    assert have == want, sorted(want - have)
    assert len(have) == 60


# --------------------------------------------------------------------------- exactness in each dtype
@pytest.mark.parametrize("family", F.VALUE_FAMILIES)
def test_values_are_exact_in_every_dtype_they_run_in(family):
    """The families whose reference is shared by the dtypes: each dtype's
    stored matrix widens back to the same values (and zeros keep their sign)."""
    seen = set()
    for c in cases_of(family):
        if (c.dt, c.nr, c.nc, c.maximize) in seen or c.nc > 1025:
            continue  # (beyond: the chain's four values again)
        seen.add((c.dt, c.nr, c.nc, c.maximize))
        for S, R in zip(F.members(*c), F.members(c.family, "f64", c.nr, c.nc, c.maximize)):
            W = F.widen(S, c.dt)
            assert np.array_equal(W, R) and np.array_equal(np.signbit(W), np.signbit(R)), c
    assert seen


# --------------------------------------------------------------------------- chain
@pytest.mark.parametrize("nr,nc", [(2, 2), (3, 9), (64, 64), (65, 65), (257, 257), (1025, 1100)])
def test_chain_is_one_search_of_nr_steps_and_one_path_of_nr_hops(nr, nc):
    for k in (0, 1, 2):
        C = F.chain(nr, nc, k)
        col, value, steps, hops = lbap_ref(C)
        assert steps == hops == nr, (k, steps, hops)
        off = int(np.flatnonzero(C[nr - 1] == 0)[0])   # where the chain's first column went
        assert np.array_equal(col, (np.roll(np.arange(nr), -1) + off) % nc) and value == 1
        assert threshold_value(C) == 1


def test_chain_members_of_the_cases():
    """The batches as the GPU runs them: every member an nr-step, nr-hop one."""
    for nr, nc in sorted({(c.nr, c.nc) for c in cases_of("chain")}):
        R = F.refs("chain", "i64", nr, nc)
        M = F.members("chain", "i64", nr, nc)
        assert [(s, h) for _, _, s, h in R] == [(S.shape[0],) * 2 for S in M]
        assert max(S.shape[0] for S in M) == nr


# --------------------------------------------------------------------------- mw (recorded)
@pytest.mark.parametrize("n,steps,hops", [(513, 386, 285), (1025, 770, 551)])
def test_recorded_machol_wien_answers(n, steps, hops):
    M = F.members("mw", "i64", n, n)
    R = F.refs("mw", "i64", n, n)
    assert len(M) == len(R)
    assert R[0][2:] == (steps, hops)
    for S, (col, value, s, h) in zip(M, R):
        assert s >= n / 2 and h >= n / 2
        assert col.dtype == np.int32 and np.array_equal(np.sort(col), np.arange(n))   # a matching
        assert S[np.arange(n), col].max() == value == threshold_value(S)               # that attains the optimum
        assert S.max() < 1 << 21 and np.array_equal(S.astype(np.float32).astype(np.int64), S)


# --------------------------------------------------------------------------- signed zeros
@pytest.mark.parametrize("nr,nc", SMALL)
@pytest.mark.parametrize("maximize", [False, True])
def test_signed_zeros_tell_a_key_that_orders_them(nr, nc, maximize):
    for S, (col, value, _, _) in zip(F.members("signed_zeros", "f64", nr, nc, maximize),
                                     F.refs("signed_zeros", "f64", nr, nc, maximize)):
        assert np.signbit(S[S == 0]).any() and not np.signbit(S[S == 0]).all()
        assert value == 0 and (col >= 0).all() and value == threshold_value(S, maximize)
        assert np.array_equal(col, lbap_ref(np.abs(S) * (-1 if maximize else 1), maximize)[0])
        below = np.where((S == 0) & np.signbit(S), -1e-300, S)   # -0.0 ordered below +0.0
        assert differs(col, lbap_ref(below, maximize)[0])


# --------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("c", cases_of("nan_patterns"), ids=F.case_id)
def test_nan_patterns_tell_a_key_without_the_nan_branch(c):
    """The NaN are forbidden pairs like the infinity.  A key that left out the
    NaN branch would order them by their bits: the ones on one side of the sign
    bit then are the best possible cost, which changes col; the others a cost
    beyond every finite one, which a feasible instance's search never takes
    (so there the largest finite value in their place changes nothing), and
    which makes the infeasible neighbour feasible."""
    M = F.members(*c)
    R = F.refs(*c)
    top = np.finfo(np.float64).max
    for k, (S, (col, value, _, _)) in enumerate(zip(M, R)):
        W = F.widen(S, c.dt)
        nan = np.isnan(W)
        U = F.as_bits(S, c.dt)
        assert set(np.unique(U[nan])) == set(F.nan_bits(c.dt)), "all four payloads"
        forbidden_inf = -np.inf if c.maximize else np.inf
        assert (W == forbidden_inf).sum() > nan.size // 8 and (W == -forbidden_inf).any()
        assert nan.sum() > nan.size // 8
        assert value == threshold_value(W, c.maximize)
        assert np.array_equal(F.widen(F.store(W, c.dt), c.dt)[~nan], W[~nan])   # exact in the dtype
        wrong = lbap_ref(F.nan_as_its_bits_order(S, c.dt, c.maximize), c.maximize)[0]
        as_finite = lbap_ref(np.where(nan, -top if c.maximize else top, W), c.maximize)[0]
        if k < len(M) - 1:
            assert (col >= 0).all() and np.isfinite(value)
            assert differs(col, wrong) and np.array_equal(col, as_finite)
        else:   # the neighbour: member 0 with one row of NaN
            assert (col == -1).all() and value == forbidden_inf
            assert nan[c.nr // 2].all() and np.array_equal(nan[np.arange(c.nr) != c.nr // 2],
                                                           np.isnan(F.widen(M[0], c.dt))[np.arange(c.nr) != c.nr // 2])
            assert (as_finite >= 0).all() and (wrong >= 0).all()


# --------------------------------------------------------------------------- random bits
@pytest.mark.parametrize("c", cases_of("random_bits"), ids=F.case_id)
def test_random_bits_content(c):
    for S, (col, value, _, _) in zip(F.members(*c), F.refs(*c)):
        W = F.widen(S, c.dt)
        assert (col >= 0).all() and np.isfinite(value), "feasible"
        assert np.isnan(W).any() and F.is_subnormal(S, c.dt).any() and (W < 0).any()
        assert value == threshold_value(W, c.maximize)
        chosen = W[np.arange(c.nr), col]
        assert value == (chosen.min() if c.maximize else chosen.max())


def test_subnormals_and_bfloat16_widen_exactly():
    for dt in F.FLOATS:
        e, m = F.LAYOUT[dt]
        U = np.array([1, (1 << m) - 1, 1 << m, (1 << (e + m)) | 1], dtype=F.UINT[dt])
        S = F.from_bits(U, dt)
        assert F.is_subnormal(S, dt).tolist() == [True, True, False, True]
        tiny = 2.0 ** (2 - (1 << (e - 1)) - m)
        assert F.widen(S, dt).tolist() == [tiny, tiny * ((1 << m) - 1), tiny * (1 << m), -tiny]


# --------------------------------------------------------------------------- split words
@pytest.mark.parametrize("c", cases_of("split_words"), ids=F.case_id)
def test_split_words_tell_a_compare_of_one_word(c):
    M = F.members(*c)
    R = F.refs(*c)
    for S, (col, value, _, _) in zip(M, R):
        assert value == threshold_value(S, c.maximize)
    if c.dt == "f64":
        for S, (col, _, _, _) in zip(M, R):
            U = S.view(np.uint64)
            assert np.unique(U >> np.uint64(33)).size == 1 and np.unique(U & np.uint64(0xFFFFFFFF)).size > S.size // 2
            assert np.array_equal(col, lbap_ref((U - U.min()).astype(np.int64), c.maximize)[0])   # the bits' own order
            assert differs(col, lbap_ref((U >> np.uint64(32)).astype(np.int64), c.maximize)[0])   # the upper word alone
        return
    h = 32 if c.dt == "i64" else 16
    hi_equal, lo_equal = M[0].astype(np.int64), M[1].astype(np.int64)
    assert np.unique(hi_equal >> h).size == 1 and np.unique(hi_equal).size > hi_equal.size // 2
    assert np.unique(lo_equal & ((1 << h) - 1)).tolist() == [(1 << (h - 1)) | 1]
    assert np.unique(lo_equal >> h).tolist() == [-2, -1, 0, 1]
    for S, (col, _, _, _) in zip(M[2:], R[2:]):   # mixed
        assert np.unique(S.astype(np.int64) >> h).tolist() == [-2, -1, 0, 1]
        for name, wrong in F.wrong_compares(S, c.dt).items():
            assert differs(col, lbap_ref(wrong, c.maximize)[0]), name
    # hi_equal: the low word alone decides, and as signed it decides otherwise
    W = F.wrong_compares(M[0], c.dt)
    assert np.array_equal(R[0][0], lbap_ref(W["low word only"], c.maximize)[0])
    assert differs(R[0][0], lbap_ref(W["low word signed"], c.maximize)[0])
    assert differs(R[0][0], lbap_ref(W["high word only"], c.maximize)[0])


# --------------------------------------------------------------------------- the rest
def test_small_ints_references_are_optimal():
    for c in cases_of("small_ints"):
        if c.dt not in ("i64", "f64"):
            continue
        for S, (col, value, _, _) in zip(F.members(*c), F.refs(*c)):
            assert np.abs(F.widen(S, c.dt)).max() <= 128 and value == threshold_value(S)
