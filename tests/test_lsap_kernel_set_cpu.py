"""CPU check of the built library's gfx950 code object, by the method of
test_kernel_resources_cpu: the LSAP kernels in it are exactly the recorded
set, tests/golden/lsap_kernel_names.txt (one mangled name per line, taken from
the build of the commit before the launchers were folded into one table per
design).  A launch table that loses an instantiation fails here before any GPU
runs, and so does one that gains some: every solve kernel costs code size and
build time.  None of them may have private (scratch) memory."""
import os

from conftest import GOLDEN
from test_kernel_resources_cpu import _kernel_meta


def test_lsap_kernels_are_the_recorded_set_without_scratch(tmp_path):
    meta = _kernel_meta(tmp_path)
    with open(os.path.join(GOLDEN, "lsap_kernel_names.txt")) as f:
        want = set(f.read().split())
    have = {k for k in meta if "lsap_" in k}
    assert want and have == want, {"lost": sorted(want - have), "extra": sorted(have - want)}
    assert not {k: v for k, v in meta.items() if k in have and v}, "kernels with private (scratch) memory"
