"""The blur kernel (csrc/png_blur_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy restatement
tests/png_blur_ref.py:
  * 8-bit HWC intermediates of 19 x 67 and 67 x 70 (partial tiles on both axes), 1 x 5, 5 x 1 and 2 x 2 (H x W), with 1, 2, 3 and 4
    channels; Gaussian ksize 3, 23 and 63 (on 19 rows radius 31 folds more than once, on the 1- and 2-pixel axes the fold is
    degenerate), sharpness 0, 0.3, 1, 1.9 and -2 (W < 3 and H < 3 included);
  * one launch holds files with different weights, so that reading another file's table shows;
  * every dtype, both layouts; a sentinel around the tensor and in the slots of skipped tasks stays; tasks that break a bound are
    skipped; fewer workgroups than tasks; other tile sizes than the host's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_blur_ref as B  # noqa: E402
import png_resize_ref as Z  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

FILL, GAP = 0xEE, 4096
SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.25)
DTYPES = ["uint", "float32", "float16", "bfloat16"]
SIZES = [(19, 67), (67, 70), (1, 5), (5, 1), (2, 2)]  # (H, W)
TILE = 32
PX_CAP, H16_CAP = 35840, 12288  # include/debig_hip.h: DEBIG_PNG_BLUR_PX_CAP, DEBIG_PNG_BLUR_H16_CAP


class BlurTask(C.Structure):  # include/debig_hip.h: debig_png_blur_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("table_off", C.c_uint64), ("k", C.c_int32), ("radius", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("tile_w", C.c_uint32),
                ("tile_h", C.c_uint32), ("out_sx", C.c_uint32), ("out_sy", C.c_uint32), ("out_sc", C.c_uint32),
                ("channels", C.c_uint8), ("colour_channels", C.c_uint8), ("dtype", C.c_uint8), ("op", C.c_uint8),
                ("a", C.c_float * 4), ("b", C.c_float * 4)]


assert C.sizeof(BlurTask) == 104
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_blur_batch.restype = C.c_int
        L.emu_png_blur_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


_FILES, _V = {}, {}


def _files(size, ch):
    """[(img8, op, ksize, value)]: every operation of the list, images that differ from file to file"""
    if (size, ch) not in _FILES:
        H, W = size
        rng = np.random.default_rng(1000 * ch + 10 * W + H)
        noise = rng.integers(0, 256, (H, W, ch), dtype=np.uint8)
        blocky = np.repeat(np.repeat(rng.integers(0, 2, (-(-H // 4), -(-W // 4), ch), dtype=np.uint8) * 255, 4, 0), 4, 1)[:H, :W]
        blocky = np.ascontiguousarray(blocky)
        ramp = ((np.arange(H)[:, None, None] * 7 + np.arange(W)[None, :, None] * 3 + np.arange(ch) * 50) % 256).astype(np.uint8)
        _FILES[(size, ch)] = [(noise, B.GAUSSIAN, 23, 2.0), (blocky, B.GAUSSIAN, 63, 10.0), (noise, B.GAUSSIAN, 3, 0.1),
                              (ramp, B.GAUSSIAN, 3, 0.8), (blocky, B.GAUSSIAN, 23, 2.0), (noise, B.GAUSSIAN, 63, 30.0),
                              (noise, B.SHARPNESS, 0, 0.0), (blocky, B.SHARPNESS, 0, 0.3), (ramp, B.SHARPNESS, 0, 1.0),
                              (noise, B.SHARPNESS, 0, 1.9), (noise, B.SHARPNESS, 0, -2.0)]
    return _FILES[(size, ch)]


def _want(size, ch, i, dtype, layout):
    """the restatement's result for file i, its integers computed once"""
    img, op, ksize, value = _files(size, ch)[i]
    if (size, ch, i) not in _V:
        _V[(size, ch, i)] = B.blur_int(img, op, ksize, value)
    out = Z.convert(_V[(size, ch, i)], 8, dtype, SCALE, BIAS)
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1))) if layout == "chw" else out


def run(files, size, dtype, layout, tile=(TILE, TILE), grid=0, spoil=None):
    """-> (the dense tensor, the number of tasks, the tasks of each file)"""
    H, W = size
    ch = files[0][0].shape[2]
    cc = B.colour_channels(ch)
    code = Z.DTYPES[dtype]
    es = 1 if code == 0 else 4 if code == 1 else 2
    slot = H * W * ch * es
    fa, fb = Z.affine(8, SCALE, BIAS)
    arena, soff = bytearray(16), []
    for img, _, _, _ in files:
        arena += bytes(-len(arena) % 16)
        soff.append(len(arena))
        arena += np.ascontiguousarray(img).tobytes()
    a = np.frombuffer(bytes(arena), np.uint8).copy()  # exactly as long as the pixels
    tables = bytearray()
    tasks, per_file = [], []
    th, tw = tile
    for i, (img, op, ksize, value) in enumerate(files):
        toff, k, r = 0, 0, 1
        if op == B.GAUSSIAN:
            toff, r = len(tables), ksize // 2
            q = B.weights(ksize, value)
            tables += np.array(q + [0] * (64 - len(q)), np.int16).tobytes()
        else:
            k = B.sharpness_k(value)
        first = len(tasks)
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                t = BlurTask(src_off=soff[i], out_off=GAP + i * slot, table_off=toff, k=k, radius=r, w=W, h=H, x0=x0, y0=y0,
                             tile_w=min(tw, W - x0), tile_h=min(th, H - y0), channels=ch, colour_channels=cc, dtype=code, op=op)
                t.out_sx, t.out_sy, t.out_sc = (1, W, H * W) if layout == "chw" else (ch, W * ch, 1)
                t.a[:] = [float(v) for v in fa]
                t.b[:] = [float(v) for v in fb]
                tasks.append(t)
        per_file.append(range(first, len(tasks)))
    if spoil:
        spoil(tasks, per_file)
    n = len(tasks)
    arr = (BlurTask * n)(*tasks)
    ta = np.frombuffer(bytes(tables), np.uint8).copy() if tables else np.zeros(16, np.uint8)
    out = np.full(GAP + len(files) * slot + GAP, FILL, np.uint8)
    assert launch("png_blur", a, out, arr, ta, n, grid, emu=_emu) == 0
    assert (out[:GAP] == FILL).all() and (out[GAP + len(files) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    npdt = {0: np.uint8, 1: np.float32, 2: np.float16, 3: np.uint16}[code]
    shape = (len(files), ch, H, W) if layout == "chw" else (len(files), H, W, ch)
    return out[GAP: GAP + len(files) * slot].view(npdt).reshape(shape), n, per_file


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_blur_kernel_against_the_reference(size, ch, layout):
    files = _files(size, ch)
    for dtype in DTYPES:
        got, n, _ = run(files, size, dtype, layout)
        assert n == len(files) * -(-size[0] // TILE) * -(-size[1] // TILE)
        for i in range(len(files)):
            want = _want(size, ch, i, dtype, layout)
            assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                (size, ch, layout, dtype, i, np.argwhere(got[i] != want)[:4])


def test_the_sources_take_every_path_of_the_rule():
    """the cases the parametrised test relies on are really there (a test of this file's own sources and of the restatement: it
    runs no project code)"""
    size, ch = SIZES[1], 4
    files = _files(size, ch)
    u8 = [_want(size, ch, i, "uint", "hwc") for i in range(len(files))]
    assert not np.array_equal(u8[0], u8[4]) and not np.array_equal(u8[0], files[0][0])  # other images, and blurred
    assert np.array_equal(u8[2], files[2][0])  # ksize 3 at sigma 0.1: the centre tap is the whole weight
    assert B.weights(3, 0.1) == [0, 16384, 0] and B.weights(23, 2.0) != B.weights(63, 10.0)[20:43]
    assert np.array_equal(u8[8], files[8][0])  # factor 1: the identity
    assert np.array_equal(u8[6][..., :3], B.smooth(files[6][0])[..., :3]) and np.array_equal(u8[6][..., 3], files[6][0][..., 3])
    assert (u8[9] == 0).any() and (u8[9] == 255).any() and (u8[10] == 0).any()  # the clamp, both ends
    v = _V[(size, ch, 0)]
    assert (v & ((1 << 22) - 1)).any()  # sub-LSB precision reaches the conversion
    assert list(B.fold(np.array([-31, -19, -18, -17, -1, 0, 18, 19, 36, 37, 48]), 19)) == [5, 17, 18, 17, 1, 0, 18, 17, 0, 1, 12]  # folds twice
    assert (B.fold(np.arange(-31, 40), 1) == 0).all() and set(B.fold(np.arange(-31, 40), 2)) == {0, 1}
    for i in (6, 9):  # W < 3 or H < 3: no interior, the sharpness result is the image
        for small in SIZES[2:]:
            assert np.array_equal(_want(small, 3, i, "uint", "hwc"), _files(small, 3)[i][0])


@pytest.mark.parametrize("tile", [(32, 64), (64, 32), (5, 17), (64, 64)])
def test_other_tiles_than_the_hosts(tile):
    """(tile_h, tile_w); a tile whose rows with the halo do not fit is skipped: take only what fits"""
    size, ch = SIZES[1], 3
    files = [f for f in _files(size, ch)
             if (min(tile[0], size[0]) + 2 * (f[2] // 2 or 1)) * (min(tile[1], size[1]) + 2 * (f[2] // 2 or 1)) * ch <= PX_CAP and
             (f[1] != B.GAUSSIAN or (min(tile[0], size[0]) + 2 * (f[2] // 2)) * min(tile[1], size[1]) * ch <= H16_CAP)]
    assert len(files) >= 5
    idx = [i for i, f in enumerate(_files(size, ch)) if any(f is g for g in files)]
    for dtype, layout in (("uint", "hwc"), ("float32", "chw")):
        got, _, _ = run(files, size, dtype, layout, tile=tile)
        for k, i in enumerate(idx):
            assert got[k].tobytes() == _want(size, ch, i, dtype, layout).tobytes(), (tile, dtype, i)


def test_fewer_workgroups_than_tasks():
    size, ch = SIZES[1], 4
    files = _files(size, ch)
    for grid in (3, 1, 7):
        got, n, _ = run(files, size, "bfloat16", "hwc", grid=grid)
        assert n > grid
        for i in range(len(files)):
            assert got[i].tobytes() == _want(size, ch, i, "bfloat16", "hwc").tobytes(), (grid, i)


def test_tasks_that_break_a_bound_are_skipped():
    size, ch = SIZES[0], 3  # 19 x 67: three tiles per file
    files = _files(size, ch)

    def spoil(tasks, per_file):
        def every(i, **kw):
            for k in per_file[i]:
                for name, val in kw.items():
                    setattr(tasks[k], name, val)
        every(0, channels=5)
        every(1, radius=32)
        every(2, colour_channels=2)
        every(3, dtype=4)
        every(4, op=3)
        every(5, table_off=tasks[per_file[5][0]].table_off + 8)
        every(6, radius=2)           # sharpness: the halo is one pixel
        every(7, k=(16 << 16) + 1)
        every(8, op=0)
        every(9, tile_h=65)
        t = tasks[per_file[10][0]]   # file 10: its first tile only
        t.x0 = 40                    # 40 + 32 > 67: it leaves the image

    got, _, per_file = run(files, size, "uint", "hwc", spoil=spoil)
    for i in range(10):
        assert (got[i] == FILL).all(), i
    want = _want(size, ch, 10, "uint", "hwc")
    assert (got[10][:, :TILE] == FILL).all() and np.array_equal(got[10][:, TILE:], want[:, TILE:])

    def spoil2(tasks, per_file):
        for k in per_file[0]:
            tasks[k].w = 16385
        for k in per_file[1]:        # (19 + 62) x (64 + 62) x 3 bytes fit, (19 + 62) x 64 x 3 halfwords do not
            tasks[k].tile_w = 64
        for k in per_file[2]:
            tasks[k].x0 = size[1]
        for k in per_file[3]:
            tasks[k].y0, tasks[k].tile_h = 10, 10
        for k in per_file[4]:
            tasks[k].tile_w = 0

    assert (19 + 62) * (64 + 62) * 3 <= PX_CAP < (19 + 62) * (64 + 62) * 4 and (19 + 62) * 64 * 3 > H16_CAP
    got, _, _ = run(files, size, "uint", "hwc", spoil=spoil2)
    for i in range(5):
        assert (got[i] == FILL).all(), i
    for i in range(5, len(files)):
        assert np.array_equal(got[i], _want(size, ch, i, "uint", "hwc")), i


def test_the_remaining_bounds():
    """the byte cap alone, the image's sizes, a zero radius, k below its range, a misaligned 2- or 4-byte pixel"""
    size, ch = SIZES[1], 4  # 67 x 70
    files = _files(size, ch)
    # radius 31, 4 channels, 64 rows: 10 columns need (64 + 62) x (10 + 62) x 4 = 36,288 bytes, 9 columns 35,784; the plane fits both
    assert 126 * 72 * 4 > PX_CAP >= 126 * 71 * 4 and 126 * 10 * 4 <= H16_CAP

    def spoil(tasks, per_file):
        def every(i, **kw):
            for k in per_file[i]:
                for name, val in kw.items():
                    setattr(tasks[k], name, val)
        every(0, h=0)
        every(1, x0=0, y0=0, tile_h=64, tile_w=10)  # (inside the image: only the byte cap is broken)
        every(2, h=16385)
        every(3, w=0)
        every(4, radius=0)
        every(5, src_off=tasks[per_file[5][0]].src_off + 2)  # (a multiple of 2, not of the 4-byte pixel)
        every(6, k=-(16 << 16) - 1)
        every(7, src_off=tasks[per_file[7][0]].src_off + 1)

    got, _, _ = run(files, size, "uint", "hwc", spoil=spoil)
    for i in range(8):
        assert (got[i] == FILL).all(), i
    for i in range(8, len(files)):
        assert np.array_equal(got[i], _want(size, ch, i, "uint", "hwc")), i
    # one column fewer fits the byte cap: the tiles are taken
    got, n, _ = run(files[1:2], size, "uint", "hwc", tile=(64, 9))
    assert n == 2 * 8 and np.array_equal(got[0], _want(size, ch, 1, "uint", "hwc"))
    # k at both ends of its range is taken (the host never makes more: |factor| <= 16)
    for k in (16 << 16, -(16 << 16)):
        def spoil_k(tasks, per_file, k=k):
            for j in per_file[0]:
                tasks[j].k = k
        got, _, _ = run(files[9:10], size, "uint", "hwc", spoil=spoil_k)
        assert np.array_equal(got[0], B.blur(files[9][0], B.SHARPNESS, 0, k / 65536.0))
    # a 2-byte pixel at an odd address
    size, ch = SIZES[0], 2
    files = _files(size, ch)

    def spoil2(tasks, per_file):
        for k in per_file[0]:
            tasks[k].src_off += 1

    got, _, _ = run(files, size, "uint", "hwc", spoil=spoil2)
    assert (got[0] == FILL).all()
    for i in range(1, len(files)):
        assert np.array_equal(got[i], _want(size, ch, i, "uint", "hwc")), i
