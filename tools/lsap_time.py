"""dev: time lsap_solve_batched_hash for a few cases on the library SANTA_HIP_LIB selects (A/B).
    python tools/lsap_time.py [NxB | NRxNCxB ...]     (default: 256x512 512x256 1024x256 256x4096)
NxB: B square n x n instances; NRxNCxB: B instances of the first nr rows of
the same nc x nc matrices (lsap_solve_batched_rect_hash)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-hungarian-method_amd"))
import torch  # noqa: E402
import santa_hip  # noqa: E402

cases = [tuple(int(x) for x in c.split("x")) for c in sys.argv[1:]] or [(256, 512), (512, 256), (1024, 256),
                                                                         (256, 4096)]
for case in cases:
    nr, (n, B) = (case[0], case[1:]) if len(case) == 3 else (None, case)

    def solve():
        if nr is None:
            santa_hip.solve_hash(7, 1 << 16, n, B)
        else:
            santa_hip.solve_hash(7, 1 << 16, n, B, nr=nr)

    solve()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    out = {"n": n, "B": B, "ms": min(ts)}
    if nr is not None:
        out = {"nr": nr, "nc": n, "B": B, "ms": min(ts)}
    print(json.dumps(out))
