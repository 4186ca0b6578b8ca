"""The two kernels of the per-image colour matrix (csrc/png_color_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against
the numpy restatement tests/png_color_ref.py:
  * debig_png_resize_color_kernel: RGB8 and RGBA8 of 70 x 37 and RGB16 / RGBA16 of 33 x 21 to 67 x 19 (two tiles in x, an odd
    width for the CHW byte stores), bilinear antialiased and NEAREST, both layouts, all four dtypes, one matrix per image, also
    with short tiles (several tasks per image in y) and fewer workgroups than tasks;
  * debig_png_warp_color_kernel: the same sources to 67 x 70 (4690 pixels: more than one 4096-pixel task, a width that does not
    divide 256), a rotation by 30 degrees with a CONSTANT border and an hflip with CLAMP, both filters;
  * the identity is the kernel without a matrix, a permutation permutes, the negative under NEAREST is M - plain;
  * a sentinel before and after the tensor stays intact; tasks that break a bound, or whose record does, are skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_ref as CR  # noqa: E402
import png_filter_ref as FR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_warp_ref as WR  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from debigulator_amd.api import png_color_matrix, png_warp_matrix  # noqa: E402

TILE_W, HQ_CAP, WX_CAP = 64, 12288, 4096  # DEBIG_PNG_RESIZE_TILE_W / _HQ_CAP / _WX_CAP
FILL, GAP = 0xEE, 4096
SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.25)
DTYPES = ["uint", "float32", "float16", "bfloat16"]


class ColorRec(C.Structure):  # include/debig_hip.h: debig_png_color_rec
    _fields_ = [("o", C.c_int64 * 3), ("k", C.c_int32 * 9), ("reserved", C.c_uint32)]


class ResizeColorTask(C.Structure):  # include/debig_hip.h: debig_png_resize_color_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("wx_off", C.c_uint64), ("wy_off", C.c_uint64),
                ("src_pitch", C.c_uint32), ("tile_x", C.c_uint32), ("tile_y", C.c_uint32), ("tile_w", C.c_uint32),
                ("tile_h", C.c_uint32), ("src_y0", C.c_uint32), ("src_rows", C.c_uint32), ("out_sx", C.c_uint32),
                ("out_sy", C.c_uint32), ("out_sc", C.c_uint32), ("channels", C.c_uint8), ("bits", C.c_uint8),
                ("dtype", C.c_uint8), ("reserved", C.c_uint8), ("a", C.c_float * 4), ("b", C.c_float * 4), ("reserved2", C.c_uint32),
                ("color_off", C.c_uint64)]


class WarpColorTask(C.Structure):  # include/debig_hip.h: debig_png_warp_color_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("m", C.c_int64 * 6), ("src_pitch", C.c_uint32),
                ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("row0", C.c_uint32),
                ("rows", C.c_uint32), ("out_sx", C.c_uint32), ("out_sy", C.c_uint32), ("out_sc", C.c_uint32), ("channels", C.c_uint8),
                ("bits", C.c_uint8), ("dtype", C.c_uint8), ("filter", C.c_uint8), ("border_mode", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("border", C.c_uint16 * 4), ("a", C.c_float * 4), ("b", C.c_float * 4), ("color_off", C.c_uint64)]


assert C.sizeof(ColorRec) == 64 and C.sizeof(ResizeColorTask) == 120 and C.sizeof(WarpColorTask) == 160
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for name in ("emu_png_resize_color_batch", "emu_png_warp_color_batch"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _records(mats, P):
    """the matrices as device records, one behind the other"""
    recs = (ColorRec * len(mats))()
    for r, M in zip(recs, mats):
        k, o = CR.quantise(M, P)
        r.k[:] = k
        r.o[:] = o
    return bytes(recs)


def _axis_table(filt, cl, L, aa):
    """the device table of one axis (include/debig_hip.h) -> (bytes, entries [(first, count)], max_taps)"""
    ax = FR.axis(filt, cl, L, aa)
    mt = max(len(w) for _, w in ax)
    hdr = np.zeros(2 + 2 * L, np.uint32)
    hdr[0], hdr[1] = mt, L
    wt = np.zeros((L, mt), np.int16)
    for X, (f, w) in enumerate(ax):
        hdr[2 + 2 * X], hdr[3 + 2 * X] = f, len(w)
        wt[X, :len(w)] = w
    b = hdr.tobytes() + wt.tobytes()
    return b + bytes((-len(b)) % 8), [(f, len(w)) for f, w in ax], mt


def _arena(srcs):
    arena, offs = bytearray(16), []
    for s in srcs:
        arena += bytes(-len(arena) % 16)
        offs.append(len(arena))
        arena += np.ascontiguousarray(s).tobytes()
    return np.frombuffer(bytes(arena), np.uint8).copy(), offs  # exactly as long as the pixels


def _view(out, n, size, ch, P, code, layout):
    H, W = size
    es = P // 8 if code == 0 else 4 if code == 1 else 2
    slot = H * W * ch * es
    assert (out[:GAP] == FILL).all() and (out[GAP + n * slot:] == FILL).all(), "the sentinel around the tensor was written"
    npdt = {0: np.uint8 if P == 8 else np.uint16, 1: np.float32, 2: np.float16, 3: np.uint16}[code]
    return out[GAP: GAP + n * slot].view(npdt).reshape((n, ch, H, W) if layout == "chw" else (n, H, W, ch))


def run_resize(srcs, mats, size, dtype, layout, filt, aa=True, tile_h=64, grid=0, spoil=None):
    """srcs: [(h, w, C) images of one C and depth]; mats: one 3 x 4 matrix per image -> the dense tensor"""
    H, W = size
    ch, P = srcs[0].shape[2], 8 * srcs[0].dtype.itemsize
    code = Z.DTYPES[dtype]
    es = P // 8 if code == 0 else 4 if code == 1 else 2
    slot = H * W * ch * es
    fa, fb = Z.affine(P, SCALE, BIAS)
    a, soff = _arena(srcs)
    weights, tables, tasks = bytearray(), {}, []

    def table(cl, L):
        if (cl, L) not in tables:
            tb, ent, mt = _axis_table(filt, cl, L, aa)
            tables[(cl, L)] = (len(weights), ent, mt)
            weights.extend(tb)
        return tables[(cl, L)]

    for s in srcs:
        table(s.shape[1], W), table(s.shape[0], H)
    rec_off = len(weights)
    weights.extend(_records(mats, P))
    for i, s in enumerate(srcs):
        h, w, _ = s.shape
        wx_off, _, mtx = table(w, W)
        wy_off, ey, mty = table(h, H)
        tw = min(W, TILE_W, WX_CAP // mtx, HQ_CAP // (mty * ch))
        y0 = 0
        while y0 < H:
            lo, hi, th = ey[y0][0], sum(ey[y0]), 1
            while y0 + th < H and th < tile_h:
                f, e = ey[y0 + th][0], sum(ey[y0 + th])
                if (max(hi, e) - min(lo, f)) * tw * ch > HQ_CAP:
                    break
                lo, hi, th = min(lo, f), max(hi, e), th + 1
            for x0 in range(0, W, tw):
                t = ResizeColorTask(src_off=soff[i], out_off=GAP + i * slot, wx_off=wx_off, wy_off=wy_off, src_pitch=w * ch, tile_x=x0,
                                    tile_y=y0, tile_w=min(tw, W - x0), tile_h=th, src_y0=lo, src_rows=hi - lo, channels=ch, bits=P,
                                    dtype=code, color_off=rec_off + 64 * i)
                t.out_sx, t.out_sy, t.out_sc = (1, W, H * W) if layout == "chw" else (ch, W * ch, 1)
                t.a[:] = [float(v) for v in fa]
                t.b[:] = [float(v) for v in fb]
                tasks.append(t)
            y0 += th
    if spoil:
        spoil(tasks)
    wa = np.frombuffer(bytes(weights), np.uint8).copy()
    out = np.full(GAP + len(srcs) * slot + GAP, FILL, np.uint8)
    n = len(tasks)
    assert launch("png_resize_color", a, out, (ResizeColorTask * n)(*tasks), wa, n, grid, emu=_emu) == 0
    return _view(out, len(srcs), size, ch, P, code, layout), n


def run_warp(srcs, mats, warps, size, dtype, layout, filt, mode, border=(0, 0, 0, 0), run=None, grid=0, spoil=None):
    H, W = size
    ch, P = srcs[0].shape[2], 8 * srcs[0].dtype.itemsize
    code = Z.DTYPES[dtype]
    es = P // 8 if code == 0 else 4 if code == 1 else 2
    slot = H * W * ch * es
    fa, fb = Z.affine(P, SCALE, BIAS)
    a, soff = _arena(srcs)
    run = run or max(1, 4096 // W)
    tasks = []
    for i, (s, m) in enumerate(zip(srcs, warps)):
        for y0 in range(0, H, run):
            t = WarpColorTask(src_off=soff[i], out_off=GAP + i * slot, src_pitch=s.shape[1] * ch, crop_w=s.shape[1], crop_h=s.shape[0],
                              out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), out_sx=1 if layout == "chw" else ch,
                              out_sy=W if layout == "chw" else W * ch, out_sc=H * W if layout == "chw" else 1, channels=ch, bits=P,
                              dtype=code, filter=filt, border_mode=mode, color_off=64 * i)
            t.m[:] = [int(v) for v in m]
            t.border[:] = [int(v) for v in border]
            t.a[:] = [float(v) for v in fa]
            t.b[:] = [float(v) for v in fb]
            tasks.append(t)
    if spoil:
        spoil(tasks)
    wa = np.frombuffer(_records(mats, P), np.uint8).copy()
    out = np.full(GAP + len(srcs) * slot + GAP, FILL, np.uint8)
    n = len(tasks)
    assert launch("png_warp_color", a, out, (WarpColorTask * n)(*tasks), wa, n, grid, emu=_emu) == 0
    return _view(out, len(srcs), size, ch, P, code, layout), n


# ---- the sources and the matrices ------------------------------------------------------------------------------------------------

def _img(rng, h, w, ch, P):
    px = rng.integers(0, 1 << P, size=(h, w, ch), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    px[: h // 3, : w // 3] = (1 << P) - 1  # saturated and empty patches: the extremes of every sum
    px[h - h // 4:, w - w // 4:] = 0
    return px


def _sources(ch, P):
    rng = np.random.default_rng(100 * ch + P)
    wh = (70, 37) if P == 8 else (33, 21)
    return [_img(rng, wh[1], wh[0], ch, P) for _ in range(3)]


def _matrices():
    """one per image, all different: a jitter, a matrix that clamps on both sides, the largest entries"""
    return [png_color_matrix(1.2, 0.8, 1.3, 17.0), np.array([[2.0, -1.5, 0.7, -0.1], [-0.6, 1.9, -0.4, 0.3], [0.2, 0.4, -2.0, 1.1]]),
            np.array([[16.0, -16.0, 16.0, -16.0], [-16.0, 16.0, -16.0, 16.0], [0.001, -0.002, 0.003, 0.5]])]


RESIZE_TO, WARP_TO = (19, 67), (70, 67)  # (H, W)
FORMATS = [(3, 8), (4, 8), (3, 16), (4, 16)]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("ch,P", FORMATS)
def test_resize_color_kernel_against_the_reference(ch, P, layout):
    srcs, mats = _sources(ch, P), _matrices()
    for filt, name in ((FR.BILINEAR, "bilinear"), (FR.NEAREST, "nearest")):
        for dtype in DTYPES:
            got, n = run_resize(srcs, mats, RESIZE_TO, dtype, layout, filt)
            assert n == 6  # two tiles in x per image
            for i, s in enumerate(srcs):
                want = CR.resize(s, RESIZE_TO, mats[i], name, dtype, True, None, SCALE, BIAS, layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (ch, P, layout, name, dtype, i, np.argwhere(got[i] != want)[:4])


def test_resize_color_short_tiles_and_fewer_workgroups_than_tasks():
    srcs, mats = _sources(4, 8), _matrices()
    want = [CR.resize(s, RESIZE_TO, M, "bilinear", "float32", True, None, SCALE, BIAS, "chw") for s, M in zip(srcs, mats)]
    for tile_h, grid in ((5, 0), (5, 4), (64, 1)):
        got, n = run_resize(srcs, mats, RESIZE_TO, "float32", "chw", FR.BILINEAR, tile_h=tile_h, grid=grid)
        assert n == (24 if tile_h == 5 else 6)
        for i in range(3):
            assert got[i].tobytes() == want[i].tobytes(), (tile_h, grid, i)


def _warps(srcs):
    return [WR.quantise([v for r in png_warp_matrix((s.shape[1], s.shape[0]), WARP_TO, angle=30.0, scale=1.7 + 0.2 * i,
                                                   translate=(1.5 * i, -2.0)) for v in r]) for i, s in enumerate(srcs)], \
           [WR.quantise([v for r in png_warp_matrix((s.shape[1], s.shape[0]), WARP_TO, hflip=True, scale=(67 / s.shape[1], 70 / s.shape[0]))
                         for v in r]) for s in srcs]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("ch,P", FORMATS)
def test_warp_color_kernel_against_the_reference(ch, P, layout):
    srcs, mats = _sources(ch, P), _matrices()
    rot, flip = _warps(srcs)
    border = [(1 << P) - 1, (1 << P) // 4, 0, (1 << P) // 2]
    for ws, mode, filt, dtypes in ((rot, WR.CONSTANT, WR.BILINEAR, DTYPES), (rot, WR.CONSTANT, WR.NEAREST, ["uint", "float32"]),
                                   (flip, WR.CLAMP, WR.BILINEAR, ["uint", "bfloat16"]), (flip, WR.CLAMP, WR.NEAREST, ["float16"])):
        for dtype in dtypes:
            got, n = run_warp(srcs, mats, ws, WARP_TO, dtype, layout, filt, mode, border)
            assert n == 6  # 61 rows of 67 pixels per task: two tasks per image
            for i, s in enumerate(srcs):
                want = CR.warp(s, WARP_TO, ws[i], mats[i], filt, dtype, mode, border, None, SCALE, BIAS, layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (ch, P, layout, filt, mode, dtype, i, np.argwhere(got[i] != want)[:4])
    # the rotation leaves the crop somewhere, so the CONSTANT border was mixed like a sample
    jx, jy = WR.picks(WARP_TO, rot[0])
    assert ((jx < 0) | (jx >= srcs[0].shape[1]) | (jy < 0) | (jy >= srcs[0].shape[0])).any()


def test_warp_color_fewer_workgroups_than_tasks_and_short_runs():
    srcs, mats = _sources(3, 16), _matrices()
    rot, _ = _warps(srcs)
    want = [CR.warp(s, WARP_TO, rot[i], mats[i], WR.BILINEAR, "float32", WR.CONSTANT, (9, 8, 7, 6), None, SCALE, BIAS, "hwc") for i, s in enumerate(srcs)]
    for run, grid in ((7, 0), (7, 5), (None, 1)):
        got, n = run_warp(srcs, mats, rot, WARP_TO, "float32", "hwc", WR.BILINEAR, WR.CONSTANT, (9, 8, 7, 6), run=run, grid=grid)
        assert n == (30 if run == 7 else 6)
        for i in range(3):
            assert got[i].tobytes() == want[i].tobytes(), (run, grid, i)


def test_exact_consequences_on_the_kernels():
    """identity == no matrix, a permutation permutes the channels (a[] / b[] stay with the output channel), the negative under
    NEAREST is M - plain"""
    for ch, P in FORMATS:
        srcs = _sources(ch, P)
        rot, _ = _warps(srcs)
        top = (1 << P) - 1
        perm = [[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]]
        order = [2, 0, 1, 3][:ch]
        for M, dtype, filt in ((CR.IDENTITY, "float32", "bilinear"), (perm, "uint", "bilinear"), (CR.NEGATIVE, "uint", "nearest")):
            got, _ = run_resize(srcs, [M] * 3, RESIZE_TO, dtype, "hwc", FR.FILTERS[filt])
            gotw, _ = run_warp(srcs, [M] * 3, rot, WARP_TO, dtype, "hwc", WR.NEAREST if filt == "nearest" else WR.BILINEAR, WR.CLAMP)
            for i, s in enumerate(srcs):
                plain = CR.resize(s, RESIZE_TO, None, filt, dtype, True, None, SCALE, BIAS, "hwc")
                plainw = CR.warp(s, WARP_TO, rot[i], None, WR.NEAREST if filt == "nearest" else WR.BILINEAR, dtype, WR.CLAMP, (0, 0, 0, 0),
                                 None, SCALE, BIAS, "hwc")
                for g, p in ((got[i], plain), (gotw[i], plainw)):
                    if M is CR.IDENTITY:
                        assert g.tobytes() == p.tobytes()
                    elif M is perm:
                        assert np.array_equal(g, p[:, :, order])
                    else:
                        assert np.array_equal(g[:, :, :3], top - p[:, :, :3]) and np.array_equal(g[:, :, 3:], p[:, :, 3:])


def test_tasks_and_records_that_break_a_bound_are_skipped():
    srcs, mats = _sources(3, 8), _matrices()
    rot, _ = _warps(srcs)

    def spoil_resize(tasks):
        tasks[0].channels = 2
        tasks[1].color_off += 4
        tasks[2].tile_w = TILE_W + 1
        tasks[3].dtype = 4

    def spoil_warp(tasks):
        tasks[0].channels = 1
        tasks[1].color_off += 4
        tasks[2].rows = WARP_TO[0] + 1
        tasks[3].bits = 12

    want = [CR.resize(s, RESIZE_TO, M, "bilinear", "uint", True, None, SCALE, BIAS, "hwc") for s, M in zip(srcs, mats)]
    got, _ = run_resize(srcs, mats, RESIZE_TO, "uint", "hwc", FR.BILINEAR, spoil=spoil_resize)
    assert (got[0] == FILL).all() and (got[1] == FILL).all() and np.array_equal(got[2], want[2])
    want = [CR.warp(s, WARP_TO, rot[i], mats[i], WR.BILINEAR, "uint", WR.CLAMP, (0, 0, 0, 0), None, SCALE, BIAS, "hwc") for i, s in enumerate(srcs)]
    got, _ = run_warp(srcs, mats, rot, WARP_TO, "uint", "hwc", WR.BILINEAR, WR.CLAMP, spoil=spoil_warp)
    assert (got[0] == FILL).all() and (got[1] == FILL).all() and np.array_equal(got[2], want[2])
    # a record beyond the quantiser's limits: its image is skipped, the others are not
    bad = [list(map(list, CR.IDENTITY)) for _ in range(3)]
    recs = bytearray(_records(bad, 8))
    r = ColorRec.from_buffer(recs, 64)
    r.k[4] = (1 << 20) + 1
    r = ColorRec.from_buffer(recs, 128)
    r.o[2] = -16 * CR.vmax(8) - 1
    orig = globals()["_records"]
    globals()["_records"] = lambda mats_, P_: bytes(recs)
    try:
        got, _ = run_resize(srcs, bad, RESIZE_TO, "uint", "hwc", FR.BILINEAR)
        gotw, _ = run_warp(srcs, bad, rot, WARP_TO, "uint", "hwc", WR.BILINEAR, WR.CLAMP)
    finally:
        globals()["_records"] = orig
    for g in (got, gotw):
        assert not (g[0] == FILL).all() and (g[1] == FILL).all() and (g[2] == FILL).all()
