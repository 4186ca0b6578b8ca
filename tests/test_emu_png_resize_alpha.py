"""The alpha resize kernel (csrc/png_resize_kernel.inc: debig_png_resize_alpha_kernel) on the CPU lock-step emulator, plain and
under ASan/UBSan, against the numpy restatement of tests/png_alpha_ref.py, BIT FOR BIT: OVER and PREMULTIPLIED x RGBA /
GRAY_ALPHA sources x 8 / 16 bit x every dtype x HWC / CHW x antialias on / off; alpha all 0, all M, hard edges and random;
backgrounds 0, M and mixed; the size, box, scale-64, tile-shape and fewer-workgroups-than-tasks cases of
test_emu_png_resize.py.  Every byte of the sentinel-filled output arena outside the written slots must stay unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as A  # noqa: E402
import png_resize_ref as Z  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402
from test_emu_png_resize import ES, FILL, HQ_CAP, SCALE, BIAS, TILE_W, WX_CAP, Task, axis_table  # noqa: E402


class AlphaTask(C.Structure):  # include/debig_hip.h: debig_png_resize_alpha_task
    _fields_ = Task._fields_ + [("mode", C.c_uint32), ("src_channels", C.c_uint8), ("out_channels", C.c_uint8),
                                ("reserved2", C.c_uint16), ("bg", C.c_uint16 * 4)]


assert C.sizeof(AlphaTask) == 128 and AlphaTask.mode.offset == 108 and AlphaTask.bg.offset == 116
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_RESIZE_EMU_ASAN") == "1")
        L.emu_png_resize_alpha_batch.restype = C.c_int
        L.emu_png_resize_alpha_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def run(images, size, mode, dtype, layout, aa, bg=(0, 0, 0), tile=(TILE_W, 64), grid=0, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0),
        gap=48):
    """images: [(px (h, w, 2 | 4) uint8 / uint16 with alpha last, box or None)], all of one channel count and depth -> the
    dense tensor as numpy (n, H, W, oc) or (n, oc, H, W); bfloat16 as bit patterns.  The tiles are sized by the SOURCE
    channel count, as the host does."""
    H, W = size
    px0 = images[0][0]
    Sc, P = px0.shape[2], 8 * px0.dtype.itemsize
    oc = Sc - 1 if mode == A.OVER else Sc
    sb = P // 8
    es = ES[dtype] or sb
    slot = H * W * oc * es
    a, b = Z.affine(P, scale, bias)
    src = bytearray(16)
    weights = bytearray()
    tables = {}
    tasks = []

    def table(cl, L):
        if (cl, L) not in tables:
            tb, ent, mt = axis_table(cl, L, aa)
            tables[(cl, L)] = (len(weights), ent, mt)
            weights.extend(tb)
        return tables[(cl, L)]

    for i, (px, box) in enumerate(images):
        h, w, _ = px.shape
        bx, by, bw, bh = box if box is not None and (box[2] or box[3]) else (0, 0, w, h)
        src += bytes((-len(src)) % 16)
        off = len(src)
        src += px.tobytes()
        wx_off, _, mtx = table(bw, W)
        wy_off, ey, mty = table(bh, H)
        tw = min(W, tile[0], TILE_W, WX_CAP // mtx, HQ_CAP // (mty * Sc))
        y0 = 0
        while y0 < H:
            lo, hi, th = ey[y0][0], sum(ey[y0]), 1
            while y0 + th < H and th < tile[1]:
                f, e = ey[y0 + th][0], sum(ey[y0 + th])
                if (max(hi, e) - min(lo, f)) * tw * Sc > HQ_CAP:
                    break
                lo, hi, th = min(lo, f), max(hi, e), th + 1
            for x0 in range(0, W, tw):
                t = AlphaTask()
                t.src_off = off + (by * w + bx) * Sc * sb
                t.out_off = gap + i * slot
                t.wx_off, t.wy_off = wx_off, wy_off
                t.src_pitch = w * Sc
                t.tile_x, t.tile_y, t.tile_w, t.tile_h = x0, y0, min(tw, W - x0), th
                t.src_y0, t.src_rows = lo, hi - lo
                t.out_sx, t.out_sy, t.out_sc = (1, W, H * W) if layout == "chw" else (oc, W * oc, 1)
                t.channels, t.bits, t.dtype = Sc, P, dtype
                t.a = (C.c_float * 4)(*a)
                t.b = (C.c_float * 4)(*b)
                t.mode, t.src_channels, t.out_channels = mode, Sc, oc
                t.bg = (C.c_uint16 * 4)(*(list(bg[:oc]) + [0] * (4 - oc) if mode == A.OVER else [0] * 4))
                tasks.append(t)
            y0 += th
    n = len(images)
    sa = np.frombuffer(bytes(src), np.uint8).copy()  # exactly as long as the pixels: a read past them is an ASan error
    wa = np.frombuffer(bytes(weights), np.uint8).copy()
    out = np.full(gap + n * slot + gap, FILL, np.uint8)
    TT = (AlphaTask * len(tasks))(*tasks)
    assert launch("png_resize_alpha", sa, out, TT, wa, len(tasks), grid, emu=_emu) == 0
    assert (out[:gap] == FILL).all() and (out[gap + n * slot:] == FILL).all(), "bytes outside the tensor were written"
    np_dt = {Z.T_UINT: np.uint8 if P == 8 else np.uint16, Z.T_F32: np.float32, Z.T_F16: np.float16, Z.T_BF16: np.uint16}[dtype]
    return out[gap: gap + n * slot].view(np_dt).reshape((n, oc, H, W) if layout == "chw" else (n, H, W, oc))


def _check(images, size, mode, dtype, layout, aa, bg=(0, 0, 0), **kw):
    got = run(images, size, mode, dtype, layout, aa, bg=bg, **kw)
    sb = {k: kw[k] for k in ("scale", "bias") if k in kw}
    for i, (px, box) in enumerate(images):
        want = A.resize_alpha(px, size, mode, dtype, aa, box, background=bg, layout=layout, **sb)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape
        assert got[i].tobytes() == want.tobytes(), (px.shape, box, size, mode, dtype, layout, aa, bg, np.argwhere(got[i] != want)[:4])


def _img(rng, h, w, Sc, P, alpha="random"):
    """colour random with saturated and empty patches; alpha: 'zero', 'full', 'edges' (0 / M blocks) or 'random'"""
    M = (1 << P) - 1
    px = rng.integers(0, M + 1, size=(h, w, Sc), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    px[: h // 3, : w // 3, :-1] = M
    px[h - h // 4:, w - w // 4:, :-1] = 0
    if alpha == "zero":
        px[:, :, -1] = 0
    elif alpha == "full":
        px[:, :, -1] = M
    elif alpha == "edges":
        y, x = np.mgrid[0:h, 0:w]
        px[:, :, -1] = np.where(((x // 5) + (y // 3)) % 2 == 0, M, 0)
    else:
        px[: h // 2, : w // 4, -1] = M  # random alpha with a saturated and an empty patch
        px[h - h // 3:, : w // 4, -1] = 0
    return px


def _bgs(P):
    M = (1 << P) - 1
    return [(0, 0, 0), (M, M, M), (M // 3, M, 1)]


MODES = [A.OVER, A.PREMULTIPLIED]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", [Z.T_UINT, Z.T_F32, Z.T_F16, Z.T_BF16])
@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("Sc", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_every_mode_source_depth_dtype_and_layout(mode, Sc, P, dtype, layout):
    rng = np.random.default_rng(mode * 1000 + Sc * 100 + P + dtype)
    for k, alpha in enumerate(("random", "edges", "zero", "full")):
        images = [(_img(rng, 23, 41, Sc, P, alpha), None), (_img(rng, 9, 7, Sc, P, alpha), None),
                  (_img(rng, 40, 30, Sc, P, alpha), (3, 5, 20, 33))]
        for aa in (True, False):
            _check(images, (11, 13), mode, dtype, layout, aa, bg=_bgs(P)[(k + aa) % 3], scale=SCALE, bias=BIAS)


@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("Sc", [2, 4])
def test_opaque_and_transparent_identities(Sc, P):
    """all M: OVER is the plain resize of the colour channels whatever the background, PREMULTIPLIED the plain resize of all
    channels; all 0: OVER is the background exactly"""
    rng = np.random.default_rng(Sc + P)
    M = (1 << P) - 1
    full, zero = _img(rng, 31, 50, Sc, P, "full"), _img(rng, 31, 50, Sc, P, "zero")
    for aa in (True, False):
        for bg in _bgs(P):
            got = run([(full, None), (zero, None)], (13, 17), A.OVER, Z.T_UINT, "hwc", aa, bg=bg)
            assert np.array_equal(got[0], Z.resize(full[:, :, :-1], (13, 17), "uint", aa))
            assert (got[1] == np.array(bg[:Sc - 1])).all()
        got = run([(full, None)], (13, 17), A.PREMULTIPLIED, Z.T_UINT, "chw", aa)
        assert np.array_equal(got[0], Z.resize(full, (13, 17), "uint", aa, layout="chw"))
    assert M == int(full[:, :, -1].max())


def test_output_sizes_1_to_70():
    rng = np.random.default_rng(2)
    images = [(_img(rng, 37, 53, 4, 8), None), (_img(rng, 5, 90, 4, 8, "edges"), None)]
    for L in range(1, 71):
        _check(images, (1 + (L * 7) % 23, L), A.OVER, Z.T_F32, "chw", L % 2 == 0, bg=(255, 128, 0), scale=SCALE, bias=BIAS)
        _check(images[:1], (L, 1 + (L * 5) % 19), MODES[L % 2], Z.T_UINT, "hwc", L % 2 == 1, bg=(7, 0, 255))


def test_224_square_across_tile_edges():
    rng = np.random.default_rng(3)
    images = [(_img(rng, 300, 517, 4, 8), None), (_img(rng, 224, 224, 4, 8, "edges"), None), (_img(rng, 97, 131, 4, 8), None)]
    _check(images, (224, 224), A.OVER, Z.T_F32, "chw", True, bg=(255, 255, 255), scale=SCALE, bias=BIAS)
    _check(images[:1], (224, 224), A.PREMULTIPLIED, Z.T_UINT, "hwc", False)


@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_source_sizes_across_tile_edges_and_one_pixel_axes(w):
    rng = np.random.default_rng(w)
    images = [(_img(rng, 1 + w % 9, w, 4, 16), None), (_img(rng, w, 1, 4, 16, "edges"), None), (_img(rng, 1, 1, 4, 16), None)]
    for size in ((64, 65), (1, 1), (5, 130)):
        _check(images, size, A.OVER, Z.T_UINT, "hwc", size != (1, 1), bg=(65535, 1, 30000))  # (antialias stops at a scale of 64)
        _check(images, size, A.PREMULTIPLIED, Z.T_BF16, "chw", False, scale=SCALE, bias=BIAS)


def test_boxes_touching_every_edge():
    rng = np.random.default_rng(6)
    W, H = 61, 47
    boxes = [(0, 0, 20, 15), (W - 20, 0, 20, 15), (0, H - 15, 20, 15), (W - 20, H - 15, 20, 15), (0, 10, W, 3), (30, 0, 2, H),
             (0, 0, W, H), (W - 1, H - 1, 1, 1), (0, 0, 0, 0), (5, 5, 1, 30)]
    for Sc, P in ((4, 8), (2, 16)):
        px = _img(rng, H, W, Sc, P)
        for aa in (True, False):
            _check([(px, b) for b in boxes], (12, 17), A.OVER, Z.T_F16, "hwc", aa, bg=_bgs(P)[2], scale=SCALE, bias=BIAS)
            _check([(px, b) for b in boxes], (25, 31), A.PREMULTIPLIED, Z.T_UINT, "chw", aa)


def test_scale_64_on_one_axis():
    rng = np.random.default_rng(7)
    a = _img(rng, 7, 64 * 3, 4, 16)   # 192 -> 3 columns: 128 horizontal taps, the narrowest tile
    b = _img(rng, 64 * 2, 50, 4, 8)   # 128 -> 2 rows: 128 vertical taps
    assert max(len(w) for _, w in Z.axis(192, 3, True)) == 128
    _check([(a, None)], (5, 3), A.OVER, Z.T_F32, "chw", True, bg=(65535, 0, 77), scale=SCALE, bias=BIAS)
    _check([(a, None)], (5, 3), A.PREMULTIPLIED, Z.T_UINT, "hwc", True)
    _check([(b, None)], (2, 70), A.PREMULTIPLIED, Z.T_F32, "hwc", True, scale=SCALE, bias=BIAS)
    _check([(b, None)], (2, 70), A.OVER, Z.T_UINT, "chw", True, bg=(255, 255, 255))
    _check([(b, None)], (2, 70), A.OVER, Z.T_UINT, "chw", False, bg=(0, 9, 255))


def test_tile_shapes_and_fewer_workgroups_than_tasks():
    rng = np.random.default_rng(8)
    images = [(_img(rng, 50, 80, 4, 8), None), (_img(rng, 33, 20, 4, 8, "edges"), (1, 2, 17, 30))]
    for k, (tile, grid) in enumerate((((7, 3), 0), ((64, 1), 5), ((1, 64), 2), ((33, 9), 1))):
        _check(images, (40, 45), MODES[k % 2], Z.T_F32, "chw", True, bg=(255, 0, 100), tile=tile, grid=grid, scale=SCALE, bias=BIAS)


def test_mismatched_tasks_are_skipped():
    """a task whose mode and channel counts do not go together, or that breaks a tile bound, writes nothing"""
    rng = np.random.default_rng(9)
    px = _img(rng, 20, 20, 4, 8)
    src = np.frombuffer(bytes(16) + px.tobytes(), np.uint8).copy()
    tb, _, _ = axis_table(20, 8, True)
    wa = np.frombuffer(tb, np.uint8).copy()
    for bad in (dict(mode=0), dict(mode=3), dict(out_channels=4), dict(src_channels=2), dict(channels=3, src_channels=3),
                dict(bits=12), dict(tile_w=65), dict(tile_w=0), dict(src_rows=400), dict(dtype=4)):
        t = AlphaTask(src_off=16, out_off=0, wx_off=0, wy_off=0, src_pitch=80, tile_x=0, tile_y=0, tile_w=8, tile_h=8, src_y0=0,
                      src_rows=20, out_sx=3, out_sy=24, out_sc=1, channels=4, bits=8, dtype=0, mode=A.OVER, src_channels=4,
                      out_channels=3)
        for k, v in bad.items():
            setattr(t, k, v)
        out = np.full(8 * 8 * 3 + 64, FILL, np.uint8)
        assert _emu().emu_png_resize_alpha_batch(src.ctypes.data, out.ctypes.data, C.byref(t), wa.ctypes.data, 1, 0) == 0
        assert (out == FILL).all(), bad


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_png_resize_alpha as E
Z, A = E.Z, E.A
rng = np.random.default_rng(21)
for Sc in (2, 4):
    for P in (8, 16):
        images = [(E._img(rng, 19, 70, Sc, P), None), (E._img(rng, 1, 1, Sc, P), None), (E._img(rng, 30, 9, Sc, P, "edges"), (2, 3, 7, 27))]
        for k, dtype in enumerate((Z.T_UINT, Z.T_F32, Z.T_F16, Z.T_BF16)):
            E._check(images, (9 + k, 66 - Sc), E.MODES[k %% 2], dtype, "chw" if (k + Sc) %% 2 else "hwc", bool((k + P // 8) %% 2),
                     bg=E._bgs(P)[k %% 3], scale=E.SCALE, bias=E.BIAS, tile=(64 - 9 * k, 5), grid=k)
E._check([(E._img(rng, 7, 192, 4, 16), None)], (5, 3), A.OVER, Z.T_F32, "chw", True, bg=(65535, 0, 5))
E._check([(E._img(rng, 128, 50, 4, 8), None)], (2, 70), A.PREMULTIPLIED, Z.T_UINT, "hwc", True)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_RESIZE_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
