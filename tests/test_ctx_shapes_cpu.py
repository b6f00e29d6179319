"""The context-shape table of tests/ctx_shapes.py on the CPU: every shape
generates, every hand-built block is a valid, non-trivial singles block, the
restated guards agree with themselves, and sh_ctx_create refuses the
arguments one past its documented limits before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

import ctx_shapes as CS
import oracle
from santa_hip import _lib


@pytest.mark.parametrize("name", CS.NAMES)
def test_shape_generates(name):
    s = CS.BY_NAME[name]
    nc = CS.nc_of(s)
    wish = np.empty((nc, s.n_wish), dtype=np.int16)
    good = np.empty((s.ng, s.n_good), dtype=np.int32)
    types = np.empty(nc, dtype=np.int16)
    rc = _lib.lib().sh_gen_synthetic(ctypes.c_uint64(5), nc, s.ng, s.nq, s.n_wish, s.n_good,
                                     wish.ctypes.data_as(ctypes.c_void_p), good.ctypes.data_as(ctypes.c_void_p),
                                     types.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    sd = CS.data(name)
    assert (sd.nc, sd.ng, sd.n_wish, sd.n_good) == (nc, s.ng, s.n_wish, s.n_good)
    assert np.array_equal(sd.types, types)
    # the block sizes of tests/test_ctx_shapes_gpu.py exist on this shape
    tri, tw = sd.families
    assert nc - tri - tw >= 8 * 256 and tw // 2 >= 2 * 256 and 50 <= CS.triplet_block_n(s) <= 64


def test_table_covers_both_sides_of_every_guard():
    S = CS.BY_NAME
    assert S["ng1022"].ng == 1022 and S["ng1023"].ng == 1023              # ng > 1022
    assert S["nw126"].n_wish == 126 and S["nw127"].n_wish == 127          # n_wish > 126
    assert CS.nc_of(S["nc2p20"]) == 1 << 20 < CS.nc_of(S["nc_over"])      # nc > 2^20
    assert CS.has_packed_copy(S["ng1024"]) and not CS.has_packed_copy(S["ng1025"])
    assert CS.has_packed_copy(S["ng1023w100"]) and not CS.has_packed_copy(S["nw126"])
    assert [CS.lattice_bound(S[k]) for k in ("nw1", "nw2", "nw3")] == [1, 3, 5]
    assert CS.lattice_bound(S["nw1"], 127) == 1 and CS.lattice_bound(S["nw2"], 127) == 3
    assert CS.lb_lds_bytes(600, 4000) <= CS.LDS_ROOM < CS.lb_lds_bytes(1025, 4000)
    assert CS.lb_lds_bytes(2000, 1000) <= CS.LDS_ROOM  # (the Kaggle shape at the reference's block size)
    assert sum(s.n_good == 1 for s in CS.SHAPES) == 1
    assert S["ng8192"].ng == 8192 and CS.largest_twins_tile_n(8192) == 243                # twins tile LDS
    # n = 244 fits the 160 KiB but not beside the kernel's static LDS: the case that found lds_room
    assert CS.twins_tile_lds_bytes(243, 8192) == 163200 <= CS.LDS_ROOM
    assert CS.LDS_ROOM < CS.twins_tile_lds_bytes(244, 8192) == 163712 <= CS.LDS_MAX
    assert CS.largest_twins_tile_n(4000) == 256 and CS.largest_twins_tile_n(1000) == 256
    for name, mode, n, B, fl, want in CS.PINS:
        assert CS.expected_design(S[name], mode, n, fl) == want, (name, mode, n, fl)


@pytest.mark.parametrize("n", [256, 600])
@pytest.mark.parametrize("name", CS.NAMES)
def test_hand_built_blocks_are_valid_and_not_trivial(name, n):
    s = CS.BY_NAME[name]
    sd = CS.data(name)
    tri, tw = sd.families
    blocks = CS.hand_blocks(s, n)
    flat = blocks.reshape(-1)
    assert np.unique(flat).size == flat.size
    assert flat.min() == tri + tw and flat.max() < sd.nc
    assert np.array_equal(np.sort(blocks[0]), np.arange(tri + tw, tri + tw + n))
    if name in CS.HIGH_ID_SHAPES:
        assert blocks.shape[0] == 2 and sd.nc - 1 in blocks[1]
        assert int((blocks[1] >= (1 << 20)).sum()) >= (200 if name == "nc_over" else 0)
        assert blocks[1].max() == (1 << 20) - 1 or name == "nc_over"
    t = sd.types.copy()
    col, _ = oracle.round_blocks(0, sd.wish, t, blocks, ng=sd.ng)
    for b in range(blocks.shape[0]):
        assert int((col[b] != np.arange(n)).sum()) >= n // 2, (name, b)
    # merged with sampled rows the blocks stay disjoint and the hand-built ones come first
    sampled = np.arange(tri + tw + 100, tri + tw + 100 + 9 * n, dtype=np.int32).reshape(9, n)
    m = CS.merge_blocks(blocks, sampled, 8)
    assert m.shape == (8, n) and np.unique(m).size == m.size
    assert np.array_equal(m[:blocks.shape[0]], blocks)


def test_static_lds_of_the_guarded_kernels(tmp_path):
    """ctx_shapes.STATIC_LDS is what the built kernels really reserve: the
    group segment's fixed size of the twins tile kernel and of every
    staged-row kernel in the library's gfx950 code object."""
    import re
    import subprocess

    from test_kernel_resources_cpu import LIB, LLVM
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or ROCm LLVM tools absent")
    fb, co = str(tmp_path / "fb.bin"), str(tmp_path / "co.o")
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fb}", LIB, str(tmp_path / "junk.so")], check=True)
    subprocess.run([tools[1], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                    f"--output={co}", "--unbundle"], check=True)
    notes = subprocess.run([tools[2], "--notes", co], check=True, capture_output=True, text=True).stdout
    static = {}
    for block in re.split(r"\n\s+- \.", notes):
        name = re.search(r"\.?name:\s+(_Z\S+)", block)
        size = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        if name and size:
            static[name.group(1)] = int(size.group(1))
    guarded = {k: v for k, v in static.items() if "santa_block_kernelILi1ELi1ELb0E" in k or "santa_lb_kernel" in k}
    assert len(guarded) >= 4, sorted(static)
    assert set(guarded.values()) == {CS.STATIC_LDS}, guarded


def _create(wish, good, nc, ng, nq=1):
    h = ctypes.c_void_p()
    wish = np.ascontiguousarray(wish, dtype=np.int16)
    good = np.ascontiguousarray(good, dtype=np.int32)
    rc = _lib.lib().sh_ctx_create(ctypes.byref(h), 0, wish.ctypes.data_as(ctypes.c_void_p), wish.shape[1],
                                  good.ctypes.data_as(ctypes.c_void_p), good.shape[1], nc, ng, nq)
    return rc, _lib.last_error()


def test_ctx_create_refuses_past_its_documented_limits_without_gpu():
    """Each refusal is decided before sh_ctx_create's first HIP call (its
    argument and table checks come first), so the code is SH_ERR_ARGS here,
    where a HIP call would fail with SH_ERR_HIP."""
    nc, ng = 400, 200
    good = np.arange(ng * 2, dtype=np.int32).reshape(ng, 2) % nc

    def wish(n_wish, width=ng):
        return (np.arange(nc)[:, None] + np.arange(n_wish)[None, :]) % width

    assert _create(wish(0), good, nc, ng) == (_lib.SH_ERR_ARGS, "n_wish must be in [1, min(127, ng)]")
    assert _create(wish(128), good, nc, ng) == (_lib.SH_ERR_ARGS, "n_wish must be in [1, min(127, ng)]")
    # n_wish > ng, at an n_wish that is otherwise fine
    g20 = np.arange(20 * 2, dtype=np.int32).reshape(20, 2)
    assert _create(wish(21, 20), g20, nc, 20) == (_lib.SH_ERR_ARGS, "n_wish must be in [1, min(127, ng)]")
    w = wish(127)
    w[nc - 1, 126] = w[nc - 1, 0]  # a repeated gift in the last row's last place
    rc, msg = _create(w, good, nc, ng)
    assert rc == _lib.SH_ERR_ARGS and "repeated gift" in msg
    g = good.copy()
    g[ng - 1, 1] = nc  # one past the last child
    rc, msg = _create(wish(127), g, nc, ng)
    assert rc == _lib.SH_ERR_ARGS and "child id out of range" in msg
    # ng: 8192 is the last accepted (decided before the tables are read)
    rc, msg = _create(wish(8), good, nc, 8193)
    assert rc == _lib.SH_ERR_ARGS and "8192" in msg
    # the limits themselves pass every host check: only the device call fails here
    for n_wish in (1, 127):
        rc, msg = _create(wish(n_wish), good, nc, ng)
        assert rc == _lib.SH_ERR_HIP, (n_wish, rc, msg)


def test_fallback_blocks_is_declared():
    assert "sh_ctx_fallback_blocks" in _lib.SIGNATURES
    assert _lib.lib().sh_ctx_fallback_blocks(None, None) == _lib.SH_ERR_ARGS
