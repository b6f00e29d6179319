"""CPU check of the built library's gfx950 code object, by the method of
test_kernel_resources_cpu: the kernels of the k-best entries (murty_*, kbest_*)
are there, the continuations are exactly launch_warm's float table up to 1024
columns for float64 and float32 costs, none keeps anything in private
(scratch) memory, and none carries `lsap_` in its mangled name (the pinned set
of tests/golden/lsap_kernel_names.txt stays what it is)."""
from test_kernel_resources_cpu import _kernel_meta


def test_kbest_kernels_exist_use_no_scratch_and_are_the_launch_table(tmp_path):
    meta = _kernel_meta(tmp_path)
    new = {k: v for k, v in meta.items() if "murty_" in k or "kbest_" in k}
    assert not [k for k in new if "lsap_" in k], "a new kernel's name contains lsap_"
    assert not {k: v for k, v in new.items() if v}, "kernels with private (scratch) memory"
    assert sum("murty_prep_kernel" in k for k in new) == 2  # float64 and float32 costs
    assert sum("kbest_pop_kernel" in k for k in new) == 1
    # one wave (one column a thread) up to 64 columns; four waves, 10-bit keys, 1 / 2 / 4 columns a thread beyond
    want = {f"murty_f64_kernelILi1E{s}E" for s in "df"}
    want |= {f"murty_f64_mw_kernelILi4ELi{k}E{s}Li10EE" for k in (1, 2, 4) for s in "df"}
    cont = [k for k in new if "murty_f64_" in k]
    assert len(cont) == 8 and len(want) == 8
    for w in want:
        assert sum(w in k for k in cont) == 1, w
    assert len(new) == 11
