"""The two kernels of the affine warp (csrc/png_warp_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy
restatement tests/png_warp_ref.py:
  * debig_png_warp_kernel: channels 1 - 4, P = 8 and 16, all four dtypes, both layouts, both filters, both border modes; crops of
    1 x 1, 1 x 9 and 13 x 7 inside a larger image, sources at odd offsets of the arena (even ones for 16-bit samples); output
    widths 1, 7, 64, 65 (the wavefront edge) and 257 (more than one pass of the workgroup along a row); several tasks per image
    whose `rows` does not divide out_h, also with fewer workgroups than tasks; the matrices of matrices() below;
  * debig_png_label_warp_kernel: 1- and 2-byte labels, with and without a LUT, all four dtypes, border_label 255 and -1;
  * a 4 KiB sentinel before and after the tensor stays intact; tasks that break a bound are skipped.
The invariants are asserted on their own: the identity is the crop, flips and quarter turns are numpy.flip / numpy.rot90, an
integer translation is the shifted crop with border, and the label pick is the image's nearest pick.  The float64 check shows
that the integer rule means what the header says (the bound is derived in png_warp_ref's docstring)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_warp_ref as WR  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from debigulator_amd.api import png_warp_matrix  # noqa: E402

FILL = 0xEE


class WarpTask(C.Structure):  # include/debig_hip.h: debig_png_warp_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("m", C.c_int64 * 6), ("src_pitch", C.c_uint32),
                ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("row0", C.c_uint32),
                ("rows", C.c_uint32), ("out_sx", C.c_uint32), ("out_sy", C.c_uint32), ("out_sc", C.c_uint32), ("channels", C.c_uint8),
                ("bits", C.c_uint8), ("dtype", C.c_uint8), ("filter", C.c_uint8), ("border_mode", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("border", C.c_uint16 * 4), ("a", C.c_float * 4), ("b", C.c_float * 4)]


class LabelWarpTask(C.Structure):  # include/debig_hip.h: debig_png_label_warp_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("m", C.c_int64 * 6), ("src_pitch", C.c_uint32),
                ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("row0", C.c_uint32),
                ("rows", C.c_uint32), ("border_label", C.c_int32), ("src_bytes", C.c_uint8), ("dtype", C.c_uint8),
                ("border_mode", C.c_uint8), ("reserved", C.c_uint8), ("reserved2", C.c_uint32)]


assert C.sizeof(WarpTask) == 152 and C.sizeof(LabelWarpTask) == 104
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_warp_batch.restype = C.c_int
        L.emu_png_warp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.emu_png_label_warp_batch.restype = C.c_int
        L.emu_png_label_warp_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + nbytes]


def _arena(srcs):
    """the sources one behind the other, each at an offset that is 1 mod 16 (one-byte samples) or 2 mod 16 (two-byte ones)"""
    arena, offs = bytearray(16), []
    for s in srcs:
        arena += bytes(-len(arena) % 16 + s.dtype.itemsize)
        offs.append(len(arena))
        arena += np.ascontiguousarray(s).tobytes() + bytes(16)
    return np.frombuffer(bytes(arena), dtype=np.uint8).copy(), offs


def _box(s, box):
    return box or (0, 0, s.shape[1], s.shape[0])


SCALE, BIAS = (1.7, 0.9, 2.2, 1.0), (-0.4, 0.1, 0.0, 0.3)


def run_warp(srcs, jobs, size, dtype="uint", layout="hwc", filt=WR.BILINEAR, mode=WR.CONSTANT, border=(0, 0, 0, 0), run=None, grid=0):
    """srcs: [(h, w, C) uint8 / uint16 images]; jobs: [(source index, box or None, m)] -> [the job's tensor, (H, W, C) or
    (C, H, W); bfloat16 as its bits].  Tasks as the host makes them (run: output rows per task, default 4096 pixels)"""
    H, W = size
    ch, P = srcs[0].shape[2], 8 * srcs[0].dtype.itemsize
    code = Z.DTYPES[dtype]
    es = P // 8 if code == 0 else 4 if code == 1 else 2
    a, soff = _arena(srcs)
    fa, fb = Z.affine(P, SCALE, BIAS)
    slot = H * W * ch * es
    run = run or max(1, 4096 // W)
    tasks = []
    for k, (si, box, m) in enumerate(jobs):
        s = srcs[si]
        x, y, bw, bh = _box(s, box)
        for y0 in range(0, H, run):
            t = WarpTask(src_off=soff[si] + (y * s.shape[1] + x) * ch * (P // 8), out_off=k * slot, src_pitch=s.shape[1] * ch,
                         crop_w=bw, crop_h=bh, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0),
                         out_sx=1 if layout == "chw" else ch, out_sy=W if layout == "chw" else W * ch,
                         out_sc=H * W if layout == "chw" else 1, channels=ch, bits=P, dtype=code, filter=filt, border_mode=mode)
            t.m[:] = [int(v) for v in m]
            t.border[:] = [int(v) for v in border]
            t.a[:] = [float(v) for v in fa]
            t.b[:] = [float(v) for v in fb]
            tasks.append(t)
    n = len(tasks)
    out = _aligned(4096 + len(jobs) * slot + 4096, FILL)
    assert launch("png_warp", a, out[4096:], (WarpTask * n)(*tasks), n, grid, emu=_emu) == 0
    assert (out[:4096] == FILL).all() and (out[4096 + len(jobs) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    npdt = {0: np.uint8 if P == 8 else np.uint16, 1: np.float32, 2: np.float16, 3: np.uint16}[code]
    shape = (len(jobs), ch, H, W) if layout == "chw" else (len(jobs), H, W, ch)
    return out[4096: 4096 + len(jobs) * slot].view(npdt).reshape(shape)


def run_label_warp(srcs, jobs, size, dtype, mode=WR.CONSTANT, border_label=0, lut=None, run=None, grid=0):
    """srcs: [(h, w) uint8 / uint16 label arrays]; jobs: [(source index, box or None, m)] -> (len(jobs), H, W) of dtype"""
    H, W = size
    es = np.dtype(LR.DTYPES[dtype]).itemsize
    a, soff = _arena(srcs)
    run = run or max(1, 4096 // W)
    tasks = []
    for k, (si, box, m) in enumerate(jobs):
        s = srcs[si]
        sb = s.dtype.itemsize
        x, y, bw, bh = _box(s, box)
        for y0 in range(0, H, run):
            t = LabelWarpTask(src_off=soff[si] + (y * s.shape[1] + x) * sb, out_off=k * H * W * es, src_pitch=s.shape[1], crop_w=bw,
                              crop_h=bh, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), border_label=border_label, src_bytes=sb,
                              dtype=list(LR.DTYPES).index(dtype), border_mode=mode)
            t.m[:] = [int(v) for v in m]
            tasks.append(t)
    n = len(tasks)
    slot = H * W * es
    out = _aligned(4096 + len(jobs) * slot + 4096, FILL)
    lt = (C.c_int32 * 256)(*[int(v) for v in lut]) if lut is not None else None
    assert launch("png_label_warp", a, out[4096:], (LabelWarpTask * n)(*tasks), lt, n, grid, emu=_emu) == 0
    assert (out[:4096] == FILL).all() and (out[4096 + len(jobs) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    return out[4096: 4096 + len(jobs) * slot].view(LR.DTYPES[dtype]).reshape(len(jobs), H, W)


# ---- the matrices ------------------------------------------------------------------------------------------------------------

def q(M):
    m = WR.quantise(M)
    assert m is not None, M
    return m


def flips_and_turns(cw, chh):
    """name -> (inverse matrix, what numpy makes of the crop (h, w, ...), output size (H, W))"""
    return {
        "identity": ((1, 0, 0, 0, 1, 0), lambda d: d, (chh, cw)),
        "hflip": ((-1, 0, cw, 0, 1, 0), lambda d: np.flip(d, 1), (chh, cw)),
        "vflip": ((1, 0, 0, 0, -1, chh), lambda d: np.flip(d, 0), (chh, cw)),
        "rot90": ((0, -1, cw, 1, 0, 0), lambda d: np.rot90(d, 1), (cw, chh)),
        "rot180": ((-1, 0, cw, 0, -1, chh), lambda d: np.rot90(d, 2), (chh, cw)),
        "rot270": ((0, 1, 0, -1, 0, chh), lambda d: np.rot90(d, 3), (cw, chh)),
    }


F_ALL_ONES = (65537 / 65536, 0, 65535 / 65536, 0, 65537 / 65536, 65535 / 65536)  # pixel (0, 0): t = 0x1FFFF on both axes


def matrices(cw, chh, size):
    """every matrix of the issue's list for a crop of cw x chh and an output of size = (H, W), quantised"""
    H, W = size
    flat = lambda M: [v for r in M for v in r]  # noqa: E731
    ms = {k: v[0] for k, v in flips_and_turns(cw, chh).items()}
    ms.update({
        "shift partly outside": (1, 0, 3, 0, 1, -2),
        "shift wholly outside x": (1, 0, cw + 5, 0, 1, 0),
        "shift wholly outside y": (1, 0, 0, 0, 1, -chh - 300),
        "30 degrees, scale 0.7": flat(png_warp_matrix((cw, chh), (H, W), angle=30, scale=0.7)),
        "zoom 40": flat(png_warp_matrix((cw, chh), (H, W), scale=40)),
        "translation +2^24": (1, 0, 2.0 ** 24, 0, 1, 2.0 ** 24),
        "translation -2^24": (1, 0, -2.0 ** 24, 0, 1, -2.0 ** 24),
        "f = 0x1FFFF": F_ALL_ONES,
        "linear entries 32768": (32768, 32768, -32768, 32768, 32768, -32768),
        "linear entries -32768": (-32768, 32768, 0.25, 32768, -32768, 0.75),
        "singular": (0, 0, 0.5, 0, 0, chh - 0.5),
    })
    return {k: q(v) for k, v in ms.items()}


def test_the_special_matrices_hit_what_they_are_for():
    U, V = WR.positions((1, 1), q(F_ALL_ONES))
    assert (int(U[0, 0]) - 65536) & 0x1FFFF == 0x1FFFF and (int(V[0, 0]) - 65536) >> 17 == 0
    assert (((int(U[0, 0]) - 65536) & 0x1FFFF) + 4) >> 3 == 16384  # w1 = 16384, w0 = 0
    m = matrices(13, 7, (7, 257))
    assert m["linear entries 32768"][:2] == [1 << 31, 1 << 31] and m["translation +2^24"][2] == 1 << 40
    U, _ = WR.positions((7, 257), m["linear entries 32768"])
    assert int(U[0, 0]) == 0 and int(np.abs(U).max()) > 1 << 40  # pixel (0, 0) inside the crop, every other one far outside


# ---- the format grid ---------------------------------------------------------------------------------------------------------

CROPS = [(1, 1), (1, 9), (13, 7)]  # (w, h), inside a 17 x 12 image
BOXES = [(16, 11, 1, 1), (5, 2, 1, 9), (3, 4, 13, 7)]
SIZES = [(1, 1), (5, 7), (7, 64), (4, 65), (5, 257)]  # (H, W): the widths of the issue's list
_SRC = {}


def _source(ch, P):
    if (ch, P) not in _SRC:
        rng = np.random.default_rng(100 * ch + P)
        s = rng.integers(0, 1 << P, size=(12, 17, ch)).astype(np.uint8 if P == 8 else np.uint16)
        s[4, 3] = (1 << P) - 1  # full scale at a crop corner
        _SRC[(ch, P)] = s
    return _SRC[(ch, P)]


@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_warp_format_grid(ch, P):
    """every dtype x layout x filter x border mode; each combination takes every matrix on one crop and one output size, and
    the crops and sizes rotate so that each meets every filter and border mode"""
    src = _source(ch, P)
    border = [(1 << P) - 1, 0, 77, 1 << (P - 1)]
    k = 0
    for dtype in Z.DTYPES:
        for layout in ("hwc", "chw"):
            for filt in (WR.BILINEAR, WR.NEAREST):
                for mode in (WR.CONSTANT, WR.CLAMP):
                    size, box = SIZES[(k + k // 5) % len(SIZES)], BOXES[k % len(BOXES)]
                    k += 1
                    ms = matrices(box[2], box[3], size)
                    jobs = [(0, box, m) for m in ms.values()]
                    got = run_warp([src], jobs, size, dtype, layout, filt, mode, border, run=3 if size[0] > 3 else None,
                                   grid=0 if k % 3 else 4)
                    for j, name in enumerate(ms):
                        exp = WR.warp(src, size, ms[name], filt, dtype, mode, border, box, SCALE, BIAS, layout)
                        assert got[j].dtype == exp.dtype and got[j].tobytes() == exp.tobytes(), \
                            (name, dtype, layout, filt, mode, size, box, np.argwhere(got[j] != exp)[:4])
    assert k == 32


@pytest.mark.parametrize("size", SIZES)
def test_every_width_on_every_crop(size):
    """RGB8 and grey 16, uint, every crop and every matrix at every output width, rows per task 2 (out_h is odd or 4)"""
    for ch, P in ((3, 8), (1, 16)):
        src = _source(ch, P)
        for box in BOXES:
            ms = matrices(box[2], box[3], size)
            for filt, mode in ((WR.BILINEAR, WR.CONSTANT), (WR.NEAREST, WR.CLAMP), (WR.BILINEAR, WR.CLAMP)):
                got = run_warp([src], [(0, box, m) for m in ms.values()], size, "uint", "hwc", filt, mode, (9, 8, 7, 6), run=2, grid=5)
                for j, name in enumerate(ms):
                    exp = WR.warp(src, size, ms[name], filt, "uint", mode, (9, 8, 7, 6), box)
                    assert np.array_equal(got[j], exp), (name, ch, P, box, filt, mode, np.argwhere(got[j] != exp)[:4])


# ---- the invariants, on their own ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [WR.BILINEAR, WR.NEAREST])
def test_identity_flips_and_quarter_turns_are_numpy(filt):
    for ch, P in ((4, 8), (3, 16), (1, 8)):
        src = _source(ch, P)
        for box in BOXES:
            x, y, bw, bh = box
            crop = src[y: y + bh, x: x + bw]
            for name, (M, fn, size) in flips_and_turns(bw, bh).items():
                for mode in (WR.CONSTANT, WR.CLAMP):
                    got = run_warp([src], [(0, box, q(M))], size, "uint", "hwc", filt, mode, (5, 5, 5, 5), run=2)[0]
                    assert np.array_equal(got, fn(crop)), (name, ch, P, box, filt, mode)
                    chw = run_warp([src], [(0, box, q(M))], size, "uint", "chw", filt, mode, (5, 5, 5, 5))[0]
                    assert np.array_equal(chw, np.transpose(fn(crop), (2, 0, 1))), (name, "chw")


@pytest.mark.parametrize("filt", [WR.BILINEAR, WR.NEAREST])
def test_integer_translations_shift_and_fill_with_border(filt):
    src = _source(3, 8)
    box = BOXES[2]
    x, y, bw, bh = box
    crop = src[y: y + bh, x: x + bw]
    border = (200, 100, 50, 0)
    for dx, dy in ((3, -2), (-5, 1), (0, 6), (bw, 0), (0, -bh), (40, 40)):
        want = np.empty_like(crop)
        want[:] = np.array(border[:3], np.uint8)
        xs, ys = np.arange(bw) + dx, np.arange(bh) + dy
        okx, oky = (xs >= 0) & (xs < bw), (ys >= 0) & (ys < bh)
        want[np.ix_(oky, okx)] = crop[np.ix_(ys[oky], xs[okx])]
        got = run_warp([src], [(0, box, q((1, 0, dx, 0, 1, dy)))], (bh, bw), "uint", "hwc", filt, WR.CONSTANT, border)[0]
        assert np.array_equal(got, want), (dx, dy, filt)
        edge = crop[np.clip(ys, 0, bh - 1)][:, np.clip(xs, 0, bw - 1)]
        got = run_warp([src], [(0, box, q((1, 0, dx, 0, 1, dy)))], (bh, bw), "uint", "hwc", filt, WR.CLAMP, border)[0]
        assert np.array_equal(got, edge), (dx, dy, filt, "clamp")


def test_the_label_pick_is_the_image_nearest_pick():
    """a source whose value encodes its own coordinates, as a two-channel 16-bit image (x, y) and as 16-bit labels
    y * 256 + x: under one matrix both kernels name the same source pixel, and border where the other has border"""
    h, w = 12, 17
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx, yy], axis=2).astype(np.uint16)
    lab = (yy * 256 + xx).astype(np.uint16)
    box = BOXES[2]
    for size in ((7, 13), (9, 65)):
        ms = matrices(box[2], box[3], size)
        jobs = [(0, box, m) for m in ms.values()]
        for mode in (WR.CONSTANT, WR.CLAMP):
            pix = run_warp([img], jobs, size, "uint", "hwc", WR.NEAREST, mode, (0xFFFF, 0xFFFF, 0, 0), run=4)
            lbl = run_label_warp([lab], jobs, size, "int32", mode, -1, run=4)
            for j, name in enumerate(ms):
                out_of_crop = lbl[j] == -1
                assert np.array_equal(out_of_crop, pix[j][:, :, 0] == 0xFFFF), name
                assert mode == WR.CONSTANT or not out_of_crop.any()
                inside = ~out_of_crop
                assert np.array_equal(lbl[j][inside], (pix[j][:, :, 1].astype(np.int32) * 256 + pix[j][:, :, 0])[inside]), name
                jx, jy = WR.picks(size, ms[name])
                ok = (jx >= 0) & (jx < box[2]) & (jy >= 0) & (jy < box[3])
                assert mode == WR.CLAMP or np.array_equal(ok, inside), name


# ---- labels --------------------------------------------------------------------------------------------------------------------

LUT = (np.random.default_rng(7).permutation(256).astype(np.int64) - 100)  # negative entries: sign extension
_LSRC = {}


def _label_sources():
    if not _LSRC:
        rng = np.random.default_rng(2)
        _LSRC[1] = rng.integers(0, 256, size=(12, 17)).astype(np.uint8)
        _LSRC[2] = rng.integers(0, 65536, size=(12, 17)).astype(np.uint16)
    return _LSRC


@pytest.mark.parametrize("dtype", list(LR.DTYPES))
def test_label_warp_every_dtype_source_lut_and_border(dtype):
    src = _label_sources()
    cases = [(1, None), (1, LUT if dtype in ("int32", "int64") else LUT + 100)]
    if dtype != "uint8":
        cases.append((2, None))
    k = 0
    for sb, lut in cases:
        for mode, bl in ((WR.CONSTANT, 255), (WR.CONSTANT, -1), (WR.CLAMP, 0)):
            if bl < 0 and dtype in ("uint8", "uint16"):
                continue  # (the host refuses it: BAD_ARG)
            for box in BOXES:
                size = SIZES[k % len(SIZES)]
                k += 1
                ms = matrices(box[2], box[3], size)
                got = run_label_warp([src[sb]], [(0, box, m) for m in ms.values()], size, dtype, mode, bl, lut, run=2, grid=k % 4)
                for j, name in enumerate(ms):
                    exp = WR.warp_labels(src[sb].astype(np.uint32), size, ms[name], mode, bl, box, lut, dtype)
                    assert got[j].dtype == exp.dtype and np.array_equal(got[j], exp), (name, dtype, sb, mode, bl, box, size)


def test_label_identity_flips_and_quarter_turns_are_numpy():
    src = _label_sources()
    for sb, dtype in ((1, "uint8"), (2, "uint16"), (1, "int64"), (2, "int32")):
        for box in BOXES:
            x, y, bw, bh = box
            crop = src[sb][y: y + bh, x: x + bw]
            for name, (M, fn, size) in flips_and_turns(bw, bh).items():
                got = run_label_warp([src[sb]], [(0, box, q(M))], size, dtype, WR.CONSTANT, 7)[0]
                assert np.array_equal(got, fn(crop)), (name, sb, dtype, box)


# ---- tasks that break a bound ----------------------------------------------------------------------------------------------------

def test_tasks_that_break_a_bound_are_skipped():
    H, W = 6, 20
    src8, src16 = _source(3, 8), _source(1, 16)
    a, soff = _arena([src8, src16])
    base = dict(src_off=soff[0], out_off=0, src_pitch=17 * 3, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, out_sx=3,
                out_sy=3 * W, out_sc=1, channels=3, bits=8, dtype=1, filter=0, border_mode=0)
    ident = [65536, 0, 0, 0, 65536, 0]
    bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
           dict(crop_h=0), dict(crop_w=1 << 31), dict(channels=0), dict(channels=5), dict(bits=12), dict(dtype=4), dict(filter=1),
           dict(filter=3), dict(border_mode=2), dict(bits=16, channels=1, src_off=soff[1] + 1)]
    tasks = []
    for b in bad:
        t = WarpTask(**dict(base, **b))
        t.m[:] = ident
        tasks.append(t)
    for k, v in ((0, (1 << 31) + 1), (1, -(1 << 31) - 1), (3, 1 << 32), (4, -(1 << 40)), (2, (1 << 40) + 1), (5, -(1 << 40) - 1)):
        t = WarpTask(**base)
        t.m[:] = ident
        t.m[k] = v
        tasks.append(t)
    out = _aligned(4096 + H * W * 3 * 4 + 4096, FILL)
    n = len(tasks)
    assert _emu().emu_png_warp_batch(a.ctypes.data, out.ctypes.data + 4096, (WarpTask * n)(*tasks), n, 0) == 0
    assert (out == FILL).all()
    ok = WarpTask(**dict(base, dtype=0))
    ok.m[:] = ident
    assert _emu().emu_png_warp_batch(a.ctypes.data, out.ctypes.data + 4096, (WarpTask * 1)(ok), 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), WR.warp(src8, (H, W), ident, WR.BILINEAR))

    lab = _label_sources()
    a, soff = _arena([lab[1], lab[2]])
    base = dict(src_off=soff[0], out_off=0, src_pitch=17, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, border_label=3,
                src_bytes=1, dtype=3, border_mode=0)
    bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
           dict(crop_h=0), dict(crop_h=1 << 31), dict(src_bytes=0), dict(src_bytes=3), dict(dtype=4), dict(dtype=0, src_bytes=2, src_off=soff[1]),
           dict(border_mode=2), dict(src_bytes=2, src_off=soff[1] + 1)]
    tasks = []
    for b in bad:
        t = LabelWarpTask(**dict(base, **b))
        t.m[:] = ident
        tasks.append(t)
    t = LabelWarpTask(**base)
    t.m[:] = [1 << 32, 0, 0, 0, 65536, 0]
    tasks.append(t)
    out = _aligned(4096 + H * W * 8 + 4096, FILL)
    n = len(tasks)
    assert _emu().emu_png_label_warp_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelWarpTask * n)(*tasks), None, n, 0) == 0
    assert (out == FILL).all()
    lt = (C.c_int32 * 256)(*range(256))  # a LUT goes with one-byte labels only
    two = LabelWarpTask(**dict(base, src_bytes=2, src_off=soff[1]))
    two.m[:] = ident
    assert _emu().emu_png_label_warp_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelWarpTask * 1)(two), lt, 1, 0) == 0
    assert (out == FILL).all()
    ok = LabelWarpTask(**base)
    ok.m[:] = ident
    assert _emu().emu_png_label_warp_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelWarpTask * 1)(ok), lt, 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W), WR.warp_labels(lab[1], (H, W), ident, WR.CONSTANT, 3))


# ---- what the integer rule means -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [8, 16])
def test_uint_bilinear_against_the_rounded_float64_map(P):
    """the kernel's UINT bilinear result against floor(float64 + 1/2) on the quantised matrix: within the bound derived in
    png_warp_ref's docstring (1 at P = 8, 5 at P = 16) -- and the bound itself is what the derivation says"""
    assert WR.float64_bound(8) == 1 and WR.float64_bound(16) == 5
    rng = np.random.default_rng(P)
    src = rng.integers(0, 1 << P, size=(23, 31, 2)).astype(np.uint8 if P == 8 else np.uint16)
    src[::3] = (1 << P) - 1  # full-scale steps: the largest |s01 - s00| the derivation allows for
    src[::3, ::2] = 0
    size = (40, 65)
    border = ((1 << P) - 1, 0, 0, 0)
    ms = matrices(31, 23, size)
    ms["7 degrees, sheared"] = q([v for r in png_warp_matrix((31, 23), size, angle=7, scale=(1.3, 0.8), shear=(5, -3), translate=(2.5, -1.25)) for v in r])
    worst = 0
    for mode in (WR.CONSTANT, WR.CLAMP):
        got = run_warp([src], [(0, None, m) for m in ms.values()], size, "uint", "hwc", WR.BILINEAR, mode, border)
        for j, name in enumerate(ms):
            ref = np.floor(WR.warp_float64(src, size, ms[name], mode, border) + 0.5).astype(np.int64)
            diff = int(np.abs(got[j].astype(np.int64) - ref).max())
            worst = max(worst, diff)
            assert diff <= WR.float64_bound(P), (name, mode, diff)
    print(f"P = {P}: largest difference to the rounded float64 map {worst}, bound {WR.float64_bound(P)}")
