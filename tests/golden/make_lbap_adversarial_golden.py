"""Writes tests/golden/lbap_adversarial.npz: lbap_ref's answers on the
Machol-Wien members of tests/lbap_families.py, whose reference loop takes
seconds an instance (513 rows: 3 s, 1025 rows: 10 s).  Per member k of
`mw` at n rows: mw_{n}_{k}_col (int16), _value (int64), _steps and _hops
(the reference's counters).  The matrices are rebuilt from lbap_families;
tests/test_lbap_adversarial_cpu.py checks each record against a live
threshold search.

    python tests/golden/make_lbap_adversarial_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lbap_families as F  # noqa: E402
from lbap_ref import lbap_ref, threshold_value  # noqa: E402


def main():
    out = {}
    for n in (513, 1025):
        for k, S in enumerate(F.members("mw", "i64", n, n)):
            col, value, steps, hops = lbap_ref(S)
            assert value == threshold_value(S)
            out[f"mw_{n}_{k}_col"] = col.astype(np.int16)
            out[f"mw_{n}_{k}_value"] = np.int64(value)
            out[f"mw_{n}_{k}_steps"] = np.int32(steps)
            out[f"mw_{n}_{k}_hops"] = np.int32(hops)
            print(n, k, int(value), steps, hops)
    np.savez_compressed(F.GOLDEN, **out)


if __name__ == "__main__":
    main()
