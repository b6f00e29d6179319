"""TEST INFRASTRUCTURE ONLY: cost-matrix families for the bottleneck solver's
witness (bneck_wit_kernel) and certificate (bneck_check_kernel), DESIGN.md §15.

Each family is built for one way the witness could be wrong and has a closed
form (col, value, wit) that needs no host loop, so it can be checked at 4096
rows; test_lbap_cert_cpu.py pins every closed form on lbap_witness_ref.

* `rise_every_search`: row i constant i.  Every search ends at once on a value
  above all earlier ones: nr rises, and the last one leaves R = {nr - 1}.
* `whole_rows`: 0 in the first nr - 1 columns, 1 beyond.  The last search walks
  through every taken column at 0 and ends on a 1: the one late rise, R = all.
* `early_rise`: row 0 constant `BIG`, the other rows whole_rows' pattern on the
  columns from 1 (2 at column 0).  Only search 0 rises; the last search visits
  every row without rising, and a stamp left by it must not reach wit: R = {0}.
* `tie_no_rewrite`: row 0 constant 5, row i 0 below the diagonal and 5 from it.
  Search i visits rows 0 .. i - 1 and ends exactly AT the running maximum: the
  strict rule keeps R = {0}, a `>=` rule returns rows 0 .. nr - 1.
* `infeasible_hall`: the last k + 1 rows are finite on the first k columns only
  (floats).  The last search fails: R = those rows, col all -1.
* `maximize_full_range`: random int64 with INT64_MIN and INT64_MAX (no closed
  form: small members for the host loop, ragged, solved with maximize).

Values are exact in all six dtypes (0, 1, 2, 5, 100, row indices below 2048 in
the narrow floats: see `fits`).  `closed_form` returns what the solver must
return; `store` / `widen` / `config_of` are lbap_families'.
"""
from __future__ import annotations

import numpy as np

from lbap_families import DTYPES, FLOATS, STORE, config_of, store, widen  # noqa: F401

BIG = 100
I64 = np.iinfo(np.int64)


def rise_every_search(nr, nc):
    return np.broadcast_to(np.arange(nr, dtype=np.int64)[:, None], (nr, nc)).copy()


def whole_rows(nr, nc):
    C = np.ones((nr, nc), dtype=np.int64)
    C[:, :nr - 1] = 0
    return C


def early_rise(nr, nc):
    C = np.ones((nr, nc), dtype=np.int64)
    C[:, 1:nr - 1] = 0
    C[:, 0] = 2
    C[0] = BIG
    return C


def tie_no_rewrite(nr, nc):
    C = np.where(np.arange(nc)[None, :] < np.arange(nr)[:, None], 0, 5).astype(np.int64)
    C[0] = 5
    return C


def infeasible_hall(nr, nc, k):
    """1 <= k < nr.  Rows 0 .. nr - k - 2: 0 at column k + i, 1 elsewhere; the
    last k + 1 rows: 0 on columns 0 .. k - 1, +inf elsewhere."""
    assert 1 <= k < nr <= nc
    C = np.ones((nr, nc), dtype=np.float64)
    i = np.arange(nr - k - 1)
    C[i, k + i] = 0
    C[nr - k - 1:] = np.inf
    C[nr - k - 1:, :k] = 0
    return C


def maximize_full_range(nr, nc, k=0):
    rng = np.random.default_rng([20251020, nr, nc, k])
    C = rng.integers(I64.min, I64.max, size=(nr, nc), endpoint=True)
    u = rng.random((nr, nc))
    C[u < 0.2] = I64.min
    C[u > 0.8] = I64.max
    return C


def closed_form(family, nr, nc, k=None):
    """-> (col int32 [nr], value (int or float), wit uint8 [nr])."""
    ident = np.arange(nr, dtype=np.int32)
    wit = np.zeros(nr, dtype=np.uint8)
    if family == "rise_every_search":
        wit[nr - 1] = 1
        return ident, nr - 1, wit
    if family == "whole_rows":
        wit[:] = 1
        assert nr >= 2  # (nr rows and nr - 1 columns of zeros: some row takes a 1)
        return ident, 1, wit
    if family == "early_rise":
        wit[0] = 1
        return ident, BIG, wit
    if family == "tie_no_rewrite":
        wit[0] = 1
        return ident, 5, wit
    if family == "infeasible_hall":
        wit[nr - k - 1:] = 1
        return np.full(nr, -1, dtype=np.int32), np.inf, wit
    raise KeyError(family)


def fits(family, dt, nr):
    """Whether every value of the family is exact in dtype dt."""
    if family == "infeasible_hall":
        return dt in FLOATS
    if family == "rise_every_search":
        return nr - 1 <= {"f16": 2048, "bf16": 256}.get(dt, 1 << 24)
    return True


# ---------------------------------------------------------------------------
# The cases of test_lbap_cert_gpu.py.  Small: (nr, nc) up to 257 columns, where
# the host loop is the reference, run in both designs; between them they reach
# (1, 1) .. (1, 8) and (4, 1), (4, 2).  Seams: square closed-form batches in the
# default design only, which reach (4, 2), (4, 4), (8, 4), (16, 4); 600 columns
# with SH_FLAG_LBAP_SW reach (1, 16).
# ---------------------------------------------------------------------------
SMALL_SHAPES = ((40, 60), (100, 128), (130, 256), (200, 257))
SEAM_SIZES = {dt: (513, 1025, 2049) + ((4096,) if dt in ("f32", "i64") else ()) for dt in DTYPES}
SW_SEAM = 600
SH_FLAG_LBAP_MW, SH_FLAG_LBAP_SW = 131072, 262144


def seam_members(dt, n):
    """[(family, k)] of the closed-form batch of dtype dt at n x n."""
    fams = [("whole_rows", None), ("early_rise", None)]
    if n == SW_SEAM:
        fams.append(("tie_no_rewrite", None))
    if dt in FLOATS:
        fams.append(("infeasible_hall", n // 3))
    elif fits("rise_every_search", dt, n):
        fams.append(("rise_every_search", None))
    return fams


def build(family, nr, nc, k=None):
    if family == "infeasible_hall":
        return infeasible_hall(nr, nc, k)
    return {"rise_every_search": rise_every_search, "whole_rows": whole_rows, "early_rise": early_rise,
            "tie_no_rewrite": tie_no_rewrite}[family](nr, nc)


# ---------------------------------------------------------------------------
# Mutations of a correct answer, each with the SH_LBCERT_ bit it must raise
# (test_lbap_cert_cpu.py proves each on lbap_check_ref; the GPU test compares
# lbap_check_ with lbap_check_ref on the same inputs).
# ---------------------------------------------------------------------------
COL, VALUE, WITNESS, NONE = 1, 2, 4, 8


def mutation_cases():
    """[(name, C, col, value, wit, maximize, bit)], all of one shape per dtype:
    int64 12 x 15 with ties and float32 12 x 15 with forbidden entries."""
    from lbap_cert_ref import lbap_witness_ref
    rng = np.random.default_rng(20251021)
    out = []
    for maximize in (False, True):
        C = rng.integers(0, 30, size=(12, 15)).astype(np.int64)
        col, value, wit = lbap_witness_ref(C, maximize)
        tag = "max-" if maximize else "min-"
        dup = col.copy()
        dup[1] = dup[0]
        out.append((tag + "duplicated column", C, dup, value, wit, maximize, COL))
        # a valid but worse assignment, with its own true value: no witness can prove it
        chosen = lambda c: C[np.arange(12), c]  # noqa: E731
        worst = (lambda x: x.min()) if maximize else (lambda x: x.max())
        while True:
            worse = rng.permutation(15)[:12].astype(np.int32)
            if worst(chosen(worse)) != value:
                break
        wv = worst(chosen(worse))
        singles = [np.eye(12, dtype=np.uint8)[i] for i in range(12)]
        for k, w in enumerate([wit, np.ones(12, dtype=np.uint8)] + singles):
            out.append((tag + f"worse assignment, witness {k}", C, worse, wv, w, maximize, WITNESS))
        best = (lambda x: x.max()) if maximize else (lambda x: x.min())
        assert best(chosen(col)) != value
        out.append((tag + "smaller value", C, col, best(chosen(col)), wit, maximize, VALUE))
        out.append((tag + "empty witness", C, col, value, np.zeros(12, dtype=np.uint8), maximize, WITNESS))
        F = rng.integers(0, 30, size=(12, 15)).astype(np.float32)
        forb = np.float32(-np.inf if maximize else np.inf)
        F[rng.random((12, 15)) < 0.3] = forb
        F[np.arange(12), rng.permutation(15)[:12]] = 1  # (feasible)
        fcol, fvalue, fwit = lbap_witness_ref(F, maximize)
        assert (fcol >= 0).all()
        for k, w in enumerate((fwit, np.ones(12, dtype=np.uint8))):
            out.append((tag + f"feasible presented as infeasible, witness {k}", F, np.full(12, -1, dtype=np.int32),
                        forb, w, maximize, WITNESS))
    return out


def configs_reached():
    """Every (NW, K, dt) that test_lbap_cert_gpu.py's cases launch."""
    out = set()
    for dt in DTYPES:
        for _, nc in SMALL_SHAPES:
            for fl in (SH_FLAG_LBAP_SW, SH_FLAG_LBAP_MW):
                out.add(config_of(nc, 4, fl) + (dt,))
        out.add(config_of(SW_SEAM, 4, SH_FLAG_LBAP_SW) + (dt,))
        for n in SEAM_SIZES[dt]:
            out.add(config_of(n, 4, 0) + (dt,))
    return out
