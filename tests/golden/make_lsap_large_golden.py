"""Generate tests/golden/lsap_large_cases.npz and lsap_large_replay.npz for the
cases of tests/lsap_large_families.py (instances above 1024 columns).  Run
where scipy is installed:

    python tests/golden/make_lsap_large_golden.py

lsap_large_cases.npz -- scipy's answers (scipy 1.15.3) on instance 0 of every
case of fixture_cases().  The matrices are not stored: the generators rebuild
them and the sha256 of the matrix bytes pins what they built.  Per case i:
`col{i}` scipy's per-row columns as int16 (-1 in every row of an infeasible
case) and meta[i]: family, dtype, nr, nc, feasible, sha.  scipy solves the
float64 image, as it does itself; the CPU oracle (oracle.lsap: int64 matrices
in exact int64) must agree before the file is written.

lsap_large_replay.npz -- lsap_duals_ref.replay (col, u, v) of the instances of
recorded_replays(), the Machol-Wien ones, whose vectorised replay takes from
seconds to half a minute each: `col{i}` int16, `u{i}`, `v{i}` in the matrix's
dtype, meta[i]: key = (family, dtype, nr, nc, k) and sha.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    from scipy.optimize import linear_sum_assignment as lsa

    import lsap_duals_ref as R
    import lsap_families as F
    import lsap_large_families as L
    import oracle
    arrays, meta = {}, []
    for family, dtype, nr, nc in L.fixture_cases():
        C = L.instance(family, dtype, nr, nc, 0)
        col = -np.ones(nr, dtype=np.int64)
        try:
            r, c = lsa(F.as_float64(C))
            col[r] = c
            feasible = True
        except ValueError:
            feasible = False
        try:  # the oracle must agree, decision for decision
            ro, co = oracle.lsap(C)
            assert feasible and np.array_equal(ro, r) and np.array_equal(co, c), (family, dtype, nr, nc)
        except ValueError:
            assert not feasible, (family, dtype, nr, nc)
        k = len(meta)
        arrays[f"col{k}"] = col.astype(np.int16)
        meta.append({"i": k, "family": family, "dtype": dtype, "nr": nr, "nc": nc, "feasible": feasible,
                     "sha": F.matrix_sha(C)})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "lsap_large_cases.npz")
    np.savez_compressed(out, **arrays)
    print(f"lsap_large_cases: {len(meta)} cases -> {out} ({os.path.getsize(out)} B)", flush=True)

    arrays, meta = {}, []
    for i, key in enumerate(L.recorded_replays()):
        C = L.instance(*key)
        col, u, v = R.replay(C)
        assert np.array_equal(col, oracle.lsap(C)[1]), key
        arrays[f"col{i}"], arrays[f"u{i}"], arrays[f"v{i}"] = col.astype(np.int16), u, v
        meta.append({"key": list(key), "sha": F.matrix_sha(C)})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "lsap_large_replay.npz")
    np.savez_compressed(out, **arrays)
    print(f"lsap_large_replay: {len(meta)} replays -> {out} ({os.path.getsize(out)} B)")


if __name__ == "__main__":
    main()
