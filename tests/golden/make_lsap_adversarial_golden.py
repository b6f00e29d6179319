"""Generate tests/golden/lsap_adversarial_cases.npz: scipy's answers (scipy
1.15.3) on the structured and extreme-value families of tests/lsap_families.py.
Run where scipy is installed:

    python tests/golden/make_lsap_adversarial_golden.py

The matrices are not stored: the generators rebuild them, and `sha{i}` (the
sha256 of the matrix bytes at its own width) pins what they built.  Per case i:
`col{i}` scipy's per-row columns as int16 (-1 in every row of an infeasible
case) and meta[i]: family, nr, nc, dtype, seed, feasible, sha.  Every matrix is
solved by scipy after conversion to float64, as scipy does itself; the CPU
oracle (oracle.lsap: int64 matrices in exact int64) must agree before the file
is written.
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

SHAPES = [(64, 64), (64, 65), (65, 65), (100, 130), (255, 256), (100, 257), (257, 257), (300, 513), (513, 513),
          (1000, 1024)]
SEED = 0


def main() -> None:
    from scipy.optimize import linear_sum_assignment as lsa

    import lsap_families as F
    import oracle
    arrays, meta = {}, []
    for family, dtype in F.all_families():
        for nr, nc in SHAPES:
            C = F.make(family, dtype, nr, nc, SEED)
            col = -np.ones(nr, dtype=np.int64)
            try:
                r, c = lsa(F.as_float64(C))
                col[r] = c
                feasible = True
            except ValueError:
                feasible = False
            Co = C if dtype == "int64" else F.as_float64(C)
            try:  # the oracle must agree, decision for decision
                ro, co = oracle.lsap(Co)
                assert feasible and np.array_equal(ro, r) and np.array_equal(co, c), (family, dtype, nr, nc)
            except ValueError:
                assert not feasible, (family, dtype, nr, nc)
            k = len(meta)
            arrays[f"col{k}"] = col.astype(np.int16)
            meta.append({"i": k, "family": family, "nr": nr, "nc": nc, "dtype": dtype, "seed": SEED,
                         "feasible": feasible, "sha": F.matrix_sha(C)})
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(HERE, "lsap_adversarial_cases.npz")
    np.savez_compressed(out, **arrays)
    bad = [(m["family"], m["dtype"], m["nr"], m["nc"]) for m in meta if not m["feasible"]]
    print(f"lsap_adversarial_cases: {len(meta)} cases ({len(bad)} infeasible: {bad}) -> {out} "
          f"({os.path.getsize(out)} B)")


if __name__ == "__main__":
    main()
