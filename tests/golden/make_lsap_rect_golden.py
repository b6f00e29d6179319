"""Generate tests/golden/lsap_rect_cases.npz: rectangular (wide and tall)
linear_sum_assignment cases with scipy's own answers (scipy 1.15.3, the
reference's LAP dependency).  Run where scipy is installed:

    python tests/golden/make_lsap_rect_golden.py

Layout as lsap_cases.npz (`meta` JSON + `C{i}` / `col{i}`) plus `row{i}`:
scipy's (row_ind, col_ind) of case i (both empty for an infeasible case).
meta[i]: nr, nc, kind ("int" / "f64-..."), hi (int cases: values in
[0, hi)), maximize, feasible, cost.  Every case is also solved by the CPU
oracle (oracle.lsap) and must agree with scipy before the file is written.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SHAPES = [(1, 1), (1, 5), (5, 1), (3, 64), (63, 65), (64, 65), (65, 64), (2, 1024), (100, 300), (300, 100)]


def main() -> None:
    from scipy.optimize import linear_sum_assignment as lsa

    import oracle
    rng = np.random.default_rng(20171226)
    arrays, meta = {}, []

    def add(C, kind, maximize=False, **extra):
        k = len(meta)
        Cs = C if C.dtype == np.float64 else C.astype(np.float64)
        Co = C if C.dtype == np.float64 else C.astype(np.int64)
        try:
            r, c = lsa(Cs, maximize=maximize)
            feasible, cost = True, float(Cs[r, c].sum())
        except ValueError:
            r = c = np.zeros(0, dtype=np.int64)
            feasible, cost = False, None
        try:  # the oracle must agree, decision for decision
            ro, co = oracle.lsap(-Co if maximize else Co)
            assert feasible and np.array_equal(ro, r) and np.array_equal(co, c), (k, kind, C.shape)
        except ValueError:
            assert not feasible, (k, kind, C.shape)
        arrays[f"C{k}"] = C
        arrays[f"row{k}"] = r.astype(np.int16)
        arrays[f"col{k}"] = c.astype(np.int16)
        meta.append({"i": k, "nr": C.shape[0], "nc": C.shape[1], "kind": kind, "maximize": maximize,
                     "feasible": feasible, "cost": cost, **extra})

    def inf_feasible(nr, nc):
        while True:  # +inf entries that leave a finite assignment
            C = rng.integers(0, 10, size=(nr, nc)).astype(np.float64)
            C[rng.random((nr, nc)) < 0.3] = np.inf
            try:
                lsa(C)
                return C
            except ValueError:
                continue

    fkinds = ("normal", "ties", "inf")
    for s, (nr, nc) in enumerate(SHAPES):
        add(rng.integers(0, 3, size=(nr, nc)).astype(np.int8), "int", hi=3)
        add(rng.integers(0, 1 << 16, size=(nr, nc)).astype(np.int32), "int", hi=1 << 16)
        # float64: arbitrary reals on the small shapes (they do not compress),
        # tie-heavy {0, 0.5, 1} and feasible +inf on the others
        fk = fkinds[s % 3] if nr * nc <= 65 * 65 else fkinds[1 + s % 2]
        if fk == "normal":
            C = rng.normal(size=(nr, nc))
        elif fk == "ties":
            C = rng.integers(0, 3, size=(nr, nc)) * 0.5
        else:
            C = inf_feasible(nr, nc)
        add(C, "f64-" + fk)
    # further float64 cases: ties and +inf, wide and tall
    add(rng.integers(0, 3, size=(63, 65)) * 0.5, "f64-ties")
    add(rng.integers(0, 3, size=(65, 64)) * 0.5, "f64-ties")
    add(inf_feasible(17, 40), "f64-inf")
    add(inf_feasible(40, 17), "f64-inf")
    # infeasible wide cases: a row of +inf; two rows whose only finite entry
    # is the same column (a Dijkstra runs dry while columns are still free)
    C = rng.integers(0, 10, size=(5, 9)).astype(np.float64)
    C[2, :] = np.inf
    add(C, "f64-infeasible-row")
    C = rng.integers(0, 10, size=(4, 8)).astype(np.float64)
    C[1, :] = np.inf
    C[3, :] = np.inf
    C[1, 5] = 2.0
    C[3, 5] = 7.0
    add(C, "f64-infeasible-pair")
    assert not meta[-1]["feasible"] and not meta[-2]["feasible"]
    # maximize: wide int, tall float64
    add(rng.integers(0, 3, size=(17, 65)).astype(np.int8), "int", maximize=True, hi=3)
    add(rng.integers(0, 3, size=(65, 17)) * 0.5, "f64-ties", maximize=True)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "lsap_rect_cases.npz")
    np.savez_compressed(out, **arrays)
    print(f"lsap_rect_cases: {len(meta)} cases -> {out} ({os.path.getsize(out)} B)")


if __name__ == "__main__":
    main()
