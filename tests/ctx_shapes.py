"""Context shapes at the edges of the Santa kernels' field widths, and the
blocks the tests run on them (plain module: no fixtures, no GPU).

Every Santa block kernel packs context-sized values into narrow fields (10-bit
gift types, 20-bit child ids, a 7-bit wish code, uint8 rank codes, int16 cost
tables of ng entries, the lattice bound M derived from the miss cost); only the
host guards of csrc/santa_api.inc keep a context of another shape away from a
kernel whose field it would overflow.  SHAPES has a context on each side of
every guard; `expected_design` restates the guards' text (pick_design,
lb_eligible, lb_lds_layout, santa_lds_layout, lds_room) so that the GPU tests compare what the library
dispatches with what the guards say, not with what the GPU returned once.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

Shape = namedtuple("Shape", "name n_wish ng nq n_good why")

SHAPES = [
    Shape("nw126", 126, 200, 150, 50, "largest wish count the 7-bit code holds: SPARSE3 still the sparse design"),
    Shape("nw127", 127, 200, 150, 50, "one past it: the sparse design is SPARSE (sp1); largest n_wish accepted"),
    Shape("nw1", 1, 300, 100, 50, "M = 1: the lattice range is not ok, every singles block takes the fallback"),
    Shape("nw2", 2, 300, 100, 50, "M = 3: the smallest ok box (|m| <= 1)"),
    Shape("nw3", 3, 300, 100, 1, "M = 5 (float32(1/6) rounds up, so 2^32 / E < 12); odd length, 2-byte loads; n_good = 1"),
    Shape("ng1022", 8, 1022, 30, 50, "last ng served by the sparse and dense-tile designs; packed copy present"),
    Shape("ng1023", 8, 1023, 30, 50, "first ng on the register tile; packed copy present, unused by the build"),
    Shape("ng1024", 8, 1024, 30, 50, "last ng with a packed copy"),
    Shape("ng1025", 8, 1025, 30, 50, "no packed copy"),
    Shape("ng1023w100", 100, 1023, 30, 50, "the ng guard with Kaggle-length wishlists (rows with 32+ hits)"),
    Shape("ng4000", 16, 4000, 8, 50, "ng-sized LDS tables: the staged-row kernel's LDS fits at n = 600, not at 1025"),
    Shape("ng8192", 64, 8192, 4, 50, "largest ng accepted: the twins tile and its chain heads no longer fit LDS at n = 256"),
    Shape("nc2p20", 8, 512, 2048, 50, "nc = 2^20 exactly: child id 2^20 - 1 must fit the 20-bit field"),
    Shape("nc_over", 8, 525, 2000, 50, "nc = 1 050 000 > 2^20: register tile; staged-row kernel ineligible"),
]
BY_NAME = {s.name: s for s in SHAPES}
NAMES = [s.name for s in SHAPES]
HIGH_ID_SHAPES = ("nc2p20", "nc_over")

# flags and designs (include/santa_hip.h; restated so that this module needs no library)
F_LDS, F_VT, F_SP, F_SP1, F_RANGE, F_DT, F_BIG = 8, 32, 128, 256, 512, 4096, 8192
SPARSE, LDS_TILE, VT_TILE, TWINS, LARGE, SPARSE3, DT_TILE, LARGE_LB = 0, 1, 3, 4, 5, 7, 8, 9

# the (mode, n, B, flag sets) every shape runs: the smallest sizes at which each
# design still runs its own code path
SINGLES_256_FLAGS = (0, F_SP, F_SP1, F_LDS, F_VT, F_DT, F_RANGE)
CASES = [
    (0, 256, 8, SINGLES_256_FLAGS),
    (0, 65, 3, (0, F_SP)),                 # one column past a wave
    (0, 600, 2, (0, F_BIG, F_RANGE)),      # staged-row kernel, or row rebuild where ineligible
    (1, 256, 2, (0, F_RANGE)),
    (1, 300, 1, (0, F_RANGE)),
]
LDS_MAX = 160 * 1024
# static LDS of the 4-wave kernels (their __syncthreads_or): what a launch's
# dynamic LDS must leave free (lds_room; tests/test_ctx_shapes_cpu.py reads it
# from the built code object)
STATIC_LDS = 256
LDS_ROOM = LDS_MAX - STATIC_LDS


def nc_of(s: Shape) -> int:
    return s.ng * s.nq


def family_sizes(nc: int):
    import math
    return math.ceil(0.005 * nc / 3.) * 3, math.ceil(0.04 * nc / 2.) * 2


def triplet_block_n(s: Shape) -> int:
    return min(64, family_sizes(nc_of(s))[0] // 3)


@functools.lru_cache(maxsize=None)
def data(name: str):
    from santa_hip import data as D
    s = BY_NAME[name]
    return D.synthetic(seed=5, nc=nc_of(s), ng=s.ng, nq=s.nq, n_wish=s.n_wish, n_good=s.n_good)


# ---------------------------------------------------------------- hand-built blocks
def low_block(s: Shape, n: int) -> np.ndarray:
    """The n lowest singles ids (right behind the families)."""
    tri, tw = family_sizes(nc_of(s))
    return np.arange(tri + tw, tri + tw + n, dtype=np.int32)


def high_block(s: Shape, n: int) -> np.ndarray:
    """The n highest child ids, nc - 1 included (descending: nc - 1 is row 0)."""
    nc = nc_of(s)
    return np.arange(nc - 1, nc - 1 - n, -1, dtype=np.int32)


def hand_blocks(s: Shape, n: int) -> np.ndarray:
    """[B, n] singles blocks the sampler will almost never pick: the lowest
    singles ids, and on the shapes that exist for them the highest child ids."""
    blocks = [low_block(s, n)]
    if s.name in HIGH_ID_SHAPES:
        blocks.append(high_block(s, n))
    return np.stack(blocks)


def merge_blocks(hand: np.ndarray, sampled: np.ndarray, B: int) -> np.ndarray:
    """[B, n] disjoint blocks: the hand-built ones first, then sampled rows
    that are in none of them (sampled: at least B blocks' worth of ids)."""
    n = hand.shape[1]
    flat = sampled.reshape(-1)
    rest = flat[~np.isin(flat, hand.reshape(-1))][:(B - hand.shape[0]) * n]
    assert rest.size == (B - hand.shape[0]) * n, "not enough sampled rows"
    return np.concatenate([hand.reshape(-1), rest]).astype(np.int32).reshape(B, n)


def block_hits(sd, rows: np.ndarray) -> np.ndarray:
    """Per row of a singles block: the columns whose gift type the row's
    child wishes (the entries of the sparse designs' hit lists)."""
    member = np.zeros((rows.size, sd.ng), dtype=bool)
    member[np.arange(rows.size)[:, None], sd.wish[rows]] = True
    return member[:, sd.types[rows]].sum(axis=1)


def sparse_blocks_left(sd, rows: np.ndarray, tile_ovf_cap: int | None, list_cap: int | None) -> int:
    """How many of rows [B, n] a sparse design leaves to its fallback launch
    for capacity: the register tile keeps 32 entries per row and spills
    entries 31.. of a longer row to an overflow list of tile_ovf_cap entries
    per block; the LDS-list kernel holds list_cap entries per block; both
    decline a block with 255+ columns of one gift type."""
    left = 0
    for r in rows:
        h = block_hits(sd, r)
        crowded = np.bincount(sd.types[r]).max() >= 255
        if tile_ovf_cap is not None:
            left += bool(crowded or int(np.where(h > 32, h - 31, 0).sum()) > tile_ovf_cap)
        else:
            left += bool(crowded or int(h.sum()) > list_cap)
    return left


# ---------------------------------------------------------------- the guards, restated
def _r16(x: int) -> int:
    return (x + 15) & ~15


def lb_lds_bytes(n: int, ng: int) -> int:
    """lb_lds_layout(n, ng, NW, K).total under with_lb_cfg's (NW, K)."""
    nw, k = (2, 4) if n <= 512 else (4, 4) if n <= 1024 else (8, 4)
    ts = ((ng + 1) & ~1) + 64 + 2
    o = _r16(n * 4) + 5 * _r16(n * 2) + _r16(n * 4) + _r16(nw * 64 * k * 2)
    o += _r16((2 * nw + 2) * ts * 2) + 32 + _r16(nw * 3 * 8)
    return o


def twins_tile_lds_bytes(n: int, ng: int) -> int:
    """santa_lds_layout(n, 1, ng).total: the 4-wave twins kernel's LDS."""
    o = _r16(n * _r16(n) * 2) + _r16(n * 8) + _r16(n * 4) + 4 * _r16(n * 2)
    o += _r16(64 * 8) + _r16(ng * 4) + _r16(n * 2) + _r16(4 * 3 * 8)
    return o


def largest_twins_tile_n(ng: int) -> int:
    """The largest n <= 256 whose twins tile fits a workgroup's LDS."""
    return max(n for n in range(1, 257) if twins_tile_lds_bytes(n, ng) <= LDS_ROOM)


def lb_eligible(s: Shape, n: int, flags: int) -> bool:
    return (256 < n <= 2048 and nc_of(s) <= (1 << 20) and not flags & F_BIG
            and lb_lds_bytes(n, s.ng) <= LDS_ROOM)


def has_packed_copy(s: Shape) -> bool:
    return s.n_wish % 4 == 0 and s.n_wish <= 102 and s.ng <= 1024


def lattice_bound(s: Shape, cap: int = 199) -> int:
    """M = min(cap, (2^32 / E) / 2), E the miss cost in units of 2^-31."""
    E = int(np.float64(np.float32(1.0 / (2.0 * s.n_wish))) * 2.0 ** 31)
    return min(cap, (0xFFFFFFFF // E) // 2)


def expected_design(s: Shape, mode: int, n: int, flags: int):
    """pick_design's answer from the guards' text: one design, or (singles
    n <= 256 on the default dispatch, where the occupancy of the dense tile
    decides) the set {DT_TILE, sparse design}."""
    if n > 256 and mode == 0 and lb_eligible(s, n, flags):
        return LARGE_LB
    if n > 256 or mode == 2:
        return LARGE
    if mode == 1:
        return TWINS if twins_tile_lds_bytes(n, s.ng) <= LDS_ROOM else LARGE
    if flags & F_LDS:
        return LDS_TILE
    if flags & F_DT:
        return DT_TILE
    if flags & F_VT or nc_of(s) > (1 << 20) or s.ng > 1022:
        return VT_TILE
    sparse = SPARSE if (s.n_wish > 126 or flags & F_SP1) else SPARSE3
    if flags & (F_SP | F_SP1):
        return sparse
    return {DT_TILE, sparse}


# The pins the module exists for, written from the guards' text (one per side
# of each guard): (shape, mode, n, B, flags) -> design.
PINS = [
    ("ng1022", 0, 256, 8, F_SP, SPARSE3),     # ng > 1022 ...
    ("ng1023", 0, 256, 8, F_SP, VT_TILE),
    ("ng1023", 0, 256, 8, 0, VT_TILE),
    ("ng1023w100", 0, 256, 8, F_SP, VT_TILE),
    ("nw126", 0, 256, 8, F_SP, SPARSE3),      # n_wish > 126 ...
    ("nw127", 0, 256, 8, F_SP, SPARSE),
    ("nc2p20", 0, 256, 8, F_SP, SPARSE3),     # nc > 2^20 ...
    ("nc_over", 0, 256, 8, F_SP, VT_TILE),
    ("nc_over", 0, 256, 8, 0, VT_TILE),
    ("nc2p20", 0, 600, 2, 0, LARGE_LB),       # lb_eligible: nc <= 2^20 ...
    ("nc_over", 0, 600, 2, 0, LARGE),
    # ... and its LDS: 2 NW + 2 tables of ng int16 each.  At ng = 4000 ten tables
    # (n = 600, four waves) take 81 KB of a 94 KB layout: eligible; eighteen
    # (n = 1025, eight waves) 146 KB of 169 KB: over the 160 KiB, row rebuild.
    ("ng4000", 0, 600, 2, 0, LARGE_LB),
    ("ng4000", 0, 1025, 1, 0, LARGE),
    ("ng4000", 0, 600, 2, F_BIG, LARGE),
    # the twins tile: 2 n r16(n) bytes beside ng chain heads.  At ng = 8192 it
    # fits up to n = 243 (163 200 of the 163 584 bytes the kernel's static LDS
    # leaves); n = 244 (163 712) fits the 160 KiB but not beside the static
    # part: row rebuild from there on.
    ("ng4000", 1, 256, 2, 0, TWINS),
    ("ng8192", 1, 243, 2, 0, TWINS),
    ("ng8192", 1, 244, 2, 0, LARGE),
    ("ng8192", 1, 256, 2, 0, LARGE),
    ("ng8192", 0, 256, 8, 0, VT_TILE),
    ("ng8192", 0, 600, 2, 0, LARGE),          # ten tables of 8192 int16: 165 KB
]
