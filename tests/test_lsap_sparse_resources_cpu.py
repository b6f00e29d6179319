"""CPU check of the built library's gfx950 code object, by the method of
test_kernel_resources_cpu: every solve kernel of the sparse (CSR) LSAP entries
is there and keeps its working set in registers and LDS (a loader with private
memory would pay a scratch round trip in every Dijkstra step)."""
from test_kernel_resources_cpu import _kernel_meta


def test_csr_solve_kernels_exist_and_use_no_scratch(tmp_path):
    meta = _kernel_meta(tmp_path)
    csr = {k: v for k, v in meta.items() if "lsap_csr_" in k}
    one = [k for k in csr if "lsap_csr_kernel" in k]
    mw = [k for k in csr if "lsap_csr_mw_kernel" in k]
    # one wave: 1 / 2 / 4 / 8 / 16 columns per thread x float64, float32 x with / without duals
    assert len(one) == 20
    # four waves (10-bit key) with 1 / 2 / 4 columns, eight waves (12-bit key) with 4 / 6 / 8: x 2 x 2
    assert sum("Li10E" in k for k in mw) == 12 and sum("Li12E" in k for k in mw) == 12 and len(mw) == 24
    assert sum("lsap_csr_prep_kernel" in k for k in csr) == 1
    assert not {k: v for k, v in csr.items() if v}, "kernels with private (scratch) memory"
