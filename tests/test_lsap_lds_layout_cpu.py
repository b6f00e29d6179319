"""The dynamic LDS bytes the LSAP launchers request are pinned by
static_asserts next to them in csrc/santa_api.inc, on the constexpr layout
functions the kernels carve from (lsap_i64_lds, lsap_f64_lds, lsap_f64_mw_lds
in csrc/santa_hip.hip).  The build checks them; this test only keeps them from
being deleted silently.

The figures are numerals worked out from the launchers' earlier hand-written
sums, not from the layout functions (r16 rounds up to 16 bytes):
  integer, 10-bit key    r16(8 nr) + r16(2 nr) + 2 r16(2 n) + 128 + 64, whatever NW
  integer, 12-bit key    r16(8 nr) + r16(2 nr) + 2 r16(2 n) + 32 NW + r16(8 NW)
  float, one wave        r16(8 nr) + r16(2 nr)
  float, NW waves        r16(8 nr) + 16 NW + r16(8 NW or, 12-bit key, 16 NW) + r16(2 nr) + 2 r16(2 n)
at the seams of the launch tables: nr = n on both sides of 64, 256, 512 and at
1 and 1024 with one and four waves; on both sides of 2048 and 3072 and at 1025
and 4096 with the (NW, key width) of the tables beyond 1024 columns; and one
rectangular shape each, nr = 1 with n at the cap.  An under-sized request does
not fault: it returns wrong assignments at the largest shapes."""
import os
import re

from conftest import ROOT

SMALL = (1, 64, 65, 256, 257, 512, 513, 1024)
I64_10 = (256, 1088, 1152, 3776, 3840, 7360, 7424, 14528)
F64 = (32, 640, 672, 2560, 2592, 5120, 5152, 10240)
F64_MW_10 = (160, 992, 1056, 3680, 3744, 7264, 7328, 14432)
LARGE = (1025, 2048, 2049, 3072, 3073, 4096)
I64_12 = ((8, 14720), (8, 28992), (16, 29376), (16, 43648), (16, 43712), (16, 57984))  # (NW, bytes)
F64_MW_12 = (14656, 28928, 28992, 43264, 43328, 57600)                                 # NW = 8


def pinned():
    for n, b in zip(SMALL, I64_10):
        yield f"lsap_i64_lds({n}, {n}, 1, 10) == {b}"
        yield f"lsap_i64_lds({n}, {n}, 4, 10) == {b}"
    for n, b, m in zip(SMALL, F64, F64_MW_10):
        yield f"lsap_f64_lds({n}) == {b}"
        yield f"lsap_f64_mw_lds({n}, {n}, 4, 10) == {m}"
    for n, (nw, b), m in zip(LARGE, I64_12, F64_MW_12):
        yield f"lsap_i64_lds({n}, {n}, {nw}, 12) == {b}"
        yield f"lsap_f64_mw_lds({n}, {n}, 8, 12) == {m}"
    yield "lsap_i64_lds(1, 1024, 4, 10) == 4320"
    yield "lsap_i64_lds(1, 4096, 16, 12) == 17056"
    yield "lsap_f64_mw_lds(1, 1024, 4, 10) == 4224"
    yield "lsap_f64_mw_lds(1, 4096, 8, 12) == 16672"


def test_requested_lds_bytes_are_pinned_by_static_asserts():
    with open(os.path.join(ROOT, "mpi-hungarian-method_amd", "csrc", "santa_api.inc")) as f:
        src = f.read()
    asserted = " ".join(re.findall(r"^static_assert\((.*)\);$", src, re.M))
    want = list(pinned())
    assert len(want) == 2 * 2 * len(SMALL) + 2 * len(LARGE) + 4
    missing = [w for w in want if w not in asserted]
    assert not missing, missing
    # and the launchers ask those functions, not a sum of their own
    lsap = src[src.index("int check_lsap_args("):]
    assert "r16(" not in lsap
    for fn in ("lsap_i64_lds(nr, n, ", "lsap_f64_lds(nr)", "lsap_f64_mw_lds(nr, n, "):
        assert fn in lsap, fn
