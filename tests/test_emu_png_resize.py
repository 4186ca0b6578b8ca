"""The resize + normalise kernel (csrc/png_resize_kernel.inc: debig_png_resize_kernel) on the CPU lock-step emulator, plain
and under ASan/UBSan, against the numpy restatement of tests/png_resize_ref.py, BIT FOR BIT: 1..4 channels x 8 / 16-bit
sources x every dtype x HWC / CHW x antialias on / off; output sizes 1..70 and one of 224 x 224, source sizes across the
tile edges, boxes touching every image edge, scale 64 on one axis, tiles of several shapes and fewer workgroups than
tasks.  Every byte of the sentinel-filled output arena outside the written slots must stay unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_resize_ref as Z  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402


class Task(C.Structure):  # include/debig_hip.h: debig_png_resize_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("wx_off", C.c_uint64), ("wy_off", C.c_uint64),
                ("src_pitch", C.c_uint32), ("tile_x", C.c_uint32), ("tile_y", C.c_uint32), ("tile_w", C.c_uint32),
                ("tile_h", C.c_uint32), ("src_y0", C.c_uint32), ("src_rows", C.c_uint32), ("out_sx", C.c_uint32),
                ("out_sy", C.c_uint32), ("out_sc", C.c_uint32), ("channels", C.c_uint8), ("bits", C.c_uint8),
                ("dtype", C.c_uint8), ("reserved", C.c_uint8), ("a", C.c_float * 4), ("b", C.c_float * 4)]


assert C.sizeof(Task) == 112
TILE_W, HQ_CAP, WX_CAP = 64, 12288, 4096  # DEBIG_PNG_RESIZE_TILE_W / _HQ_CAP / _WX_CAP
FILL = 0xEE
ES = {Z.T_UINT: None, Z.T_F32: 4, Z.T_F16: 2, Z.T_BF16: 2}
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_RESIZE_EMU_ASAN") == "1")
        L.emu_png_resize_batch.restype = C.c_int
        L.emu_png_resize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def axis_table(cl, L, aa):
    """the device table of one axis (include/debig_hip.h) -> (bytes, entries [(first, count)], max_taps)"""
    ax = Z.axis(cl, L, aa)
    mt = max(len(w) for _, w in ax)
    hdr = np.zeros(2 + 2 * L, np.uint32)
    hdr[0], hdr[1] = mt, L
    wt = np.zeros((L, mt), np.int16)
    for X, (f, w) in enumerate(ax):
        hdr[2 + 2 * X], hdr[3 + 2 * X] = f, len(w)
        wt[X, :len(w)] = w
    b = hdr.tobytes() + wt.tobytes()
    return b + bytes((-len(b)) % 8), [(f, len(w)) for f, w in ax], mt


def run(images, size, dtype, layout, aa, tile=(TILE_W, 64), grid=0, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0), gap=48):
    """images: [(px (h, w, C) uint8 / uint16, box or None)], all of one C and depth -> the dense tensor as numpy
    (n, H, W, C) or (n, C, H, W); bfloat16 as bit patterns"""
    H, W = size
    px0 = images[0][0]
    Cn, P = px0.shape[2], 8 * px0.dtype.itemsize
    sb = P // 8
    es = ES[dtype] or sb
    slot = H * W * Cn * es
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
        tw = min(W, tile[0], TILE_W, WX_CAP // mtx, HQ_CAP // (mty * Cn))
        y0 = 0
        while y0 < H:
            lo, hi, th = ey[y0][0], sum(ey[y0]), 1
            while y0 + th < H and th < tile[1]:
                f, e = ey[y0 + th][0], sum(ey[y0 + th])
                if (max(hi, e) - min(lo, f)) * tw * Cn > HQ_CAP:
                    break
                lo, hi, th = min(lo, f), max(hi, e), th + 1
            for x0 in range(0, W, tw):
                t = Task()
                t.src_off = off + (by * w + bx) * Cn * sb
                t.out_off = gap + i * slot
                t.wx_off, t.wy_off = wx_off, wy_off
                t.src_pitch = w * Cn
                t.tile_x, t.tile_y, t.tile_w, t.tile_h = x0, y0, min(tw, W - x0), th
                t.src_y0, t.src_rows = lo, hi - lo
                t.out_sx, t.out_sy, t.out_sc = (1, W, H * W) if layout == "chw" else (Cn, W * Cn, 1)
                t.channels, t.bits, t.dtype = Cn, P, dtype
                t.a = (C.c_float * 4)(*a)
                t.b = (C.c_float * 4)(*b)
                tasks.append(t)
            y0 += th
    n = len(images)
    sa = np.frombuffer(bytes(src), np.uint8).copy()  # exactly as long as the pixels: a read past them is an ASan error
    wa = np.frombuffer(bytes(weights), np.uint8).copy()
    out = np.full(gap + n * slot + gap, FILL, np.uint8)
    TT = (Task * len(tasks))(*tasks)
    assert launch("png_resize", sa, out, TT, wa, len(tasks), grid, emu=_emu) == 0
    assert (out[:gap] == FILL).all() and (out[gap + n * slot:] == FILL).all(), "bytes outside the tensor were written"
    np_dt = {Z.T_UINT: np.uint8 if P == 8 else np.uint16, Z.T_F32: np.float32, Z.T_F16: np.float16, Z.T_BF16: np.uint16}[dtype]
    return out[gap: gap + n * slot].view(np_dt).reshape((n, Cn, H, W) if layout == "chw" else (n, H, W, Cn))


def _same(got, want):
    return got.tobytes() == want.tobytes()  # bit for bit (floats as their bits, -0.0 != 0.0)


def _check(images, size, dtype, layout, aa, **kw):
    got = run(images, size, dtype, layout, aa, **kw)
    sb = {k: kw[k] for k in ("scale", "bias") if k in kw}
    for i, (px, box) in enumerate(images):
        want = Z.resize(px, size, dtype, aa, box, layout=layout, **sb)
        assert got[i].dtype == want.dtype and got[i].shape == want.shape
        assert _same(got[i], want), (px.shape, box, size, dtype, layout, aa, np.argwhere(got[i] != want)[:4])


def _img(rng, h, w, Cn, P):
    px = rng.integers(0, 1 << P, size=(h, w, Cn), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    px[: h // 3, : w // 3] = (1 << P) - 1  # saturated and empty patches: the extremes of every sum
    px[h - h // 4:, w - w // 4:] = 0
    return px


SCALE, BIAS = (1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.25)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("dtype", [Z.T_UINT, Z.T_F32, Z.T_F16, Z.T_BF16])
@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("Cn", [1, 2, 3, 4])
def test_every_channel_count_depth_dtype_and_layout(Cn, P, dtype, layout):
    rng = np.random.default_rng(Cn * 100 + P + dtype)
    images = [(_img(rng, 23, 41, Cn, P), None), (_img(rng, 9, 7, Cn, P), None), (_img(rng, 40, 30, Cn, P), (3, 5, 20, 33))]
    for aa in (True, False):
        _check(images, (11, 13), dtype, layout, aa, scale=SCALE, bias=BIAS)


def test_output_sizes_1_to_70():
    rng = np.random.default_rng(2)
    images = [(_img(rng, 37, 53, 3, 8), None), (_img(rng, 5, 90, 3, 8), None)]
    for L in range(1, 71):
        _check(images, (1 + (L * 7) % 23, L), Z.T_F32, "chw", L % 2 == 0, scale=SCALE, bias=BIAS)
        _check(images[:1], (L, 1 + (L * 5) % 19), Z.T_UINT, "hwc", L % 2 == 1)


def test_224_square_across_tile_edges():
    rng = np.random.default_rng(3)
    images = [(_img(rng, 300, 517, 3, 8), None), (_img(rng, 224, 224, 3, 8), None), (_img(rng, 97, 131, 3, 8), None)]
    _check(images, (224, 224), Z.T_F32, "chw", True, scale=SCALE, bias=BIAS)
    _check(images[:1], (224, 224), Z.T_UINT, "hwc", False)


@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_source_sizes_across_tile_edges_and_one_pixel_axes(w):
    rng = np.random.default_rng(w)
    images = [(_img(rng, 1 + w % 9, w, 4, 16), None), (_img(rng, w, 1, 4, 16), None), (_img(rng, 1, 1, 4, 16), None)]
    for size in ((64, 65), (1, 1), (5, 130)):
        _check(images, size, Z.T_UINT, "hwc", size != (1, 1))  # (antialias is refused beyond a scale of 64)
        _check(images, size, Z.T_BF16, "chw", False, scale=SCALE, bias=BIAS)


def test_identity_size_is_the_crop_exactly():
    rng = np.random.default_rng(5)
    for P in (8, 16):
        px = _img(rng, 70, 90, 3, P)
        for aa in (True, False):
            got = run([(px, None), (px, None)], (70, 90), Z.T_UINT, "hwc", aa)
            assert np.array_equal(got[0], px) and np.array_equal(got[1], px)
            got = run([(px, (10, 20, 33, 44))], (44, 33), Z.T_UINT, "chw", aa)
            assert np.array_equal(got[0], np.transpose(px[20:64, 10:43], (2, 0, 1)))


def test_boxes_touching_every_edge():
    rng = np.random.default_rng(6)
    W, H = 61, 47
    px = _img(rng, H, W, 3, 8)
    boxes = [(0, 0, 20, 15), (W - 20, 0, 20, 15), (0, H - 15, 20, 15), (W - 20, H - 15, 20, 15), (0, 10, W, 3), (30, 0, 2, H),
             (0, 0, W, H), (W - 1, H - 1, 1, 1), (0, 0, 0, 0), (5, 5, 1, 30)]
    for aa in (True, False):
        _check([(px, b) for b in boxes], (12, 17), Z.T_F16, "hwc", aa, scale=SCALE, bias=BIAS)
        _check([(px, b) for b in boxes], (25, 31), Z.T_UINT, "chw", aa)


def test_scale_64_on_one_axis():
    rng = np.random.default_rng(7)
    a = _img(rng, 7, 64 * 3, 4, 16)   # 192 -> 3 columns: 128 horizontal taps, the narrowest tile
    b = _img(rng, 64 * 2, 50, 4, 8)   # 128 -> 2 rows: 128 vertical taps
    assert max(len(w) for _, w in Z.axis(192, 3, True)) == 128
    _check([(a, None)], (5, 3), Z.T_F32, "chw", True, scale=SCALE, bias=BIAS)
    _check([(a, None)], (5, 3), Z.T_UINT, "hwc", True)
    _check([(b, None)], (2, 70), Z.T_F32, "hwc", True, scale=SCALE, bias=BIAS)
    _check([(b, None)], (2, 70), Z.T_UINT, "chw", True)
    _check([(b, None)], (2, 70), Z.T_UINT, "chw", False)


def test_tile_shapes_and_fewer_workgroups_than_tasks():
    rng = np.random.default_rng(8)
    images = [(_img(rng, 50, 80, 3, 8), None), (_img(rng, 33, 20, 3, 8), (1, 2, 17, 30))]
    for tile, grid in (((7, 3), 0), ((64, 1), 5), ((1, 64), 2), ((33, 9), 1)):
        _check(images, (40, 45), Z.T_F32, "chw", True, tile=tile, grid=grid, scale=SCALE, bias=BIAS)


def test_float16_conversion_overflow_and_subnormals():
    """scales that push the float32 result through float16's subnormals, its largest finite value and infinity"""
    rng = np.random.default_rng(9)
    px = _img(rng, 16, 16, 1, 16)
    px[0, :8, 0] = [0, 1, 2, 3, 5, 65535, 65534, 32768]
    for s, b in ((65504.0, 0.0), (65520.0, 0.0), (70000.0, -3.0), (6.2e-5, 0.0), (6e-8, 0.0), (1.2e-7, 0.0), (1e-3, -5e-4)):
        for dtype in (Z.T_F16, Z.T_BF16, Z.T_F32):
            _check([(px, None)], (16, 16), dtype, "hwc", False, scale=(s,) * 4, bias=(b,) * 4)
            _check([(px, None)], (5, 7), dtype, "hwc", True, scale=(s,) * 4, bias=(b,) * 4)


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_png_resize as E
Z = E.Z
rng = np.random.default_rng(21)
for Cn in (1, 2, 3, 4):
    for P in (8, 16):
        images = [(E._img(rng, 19, 70, Cn, P), None), (E._img(rng, 1, 1, Cn, P), None), (E._img(rng, 30, 9, Cn, P), (2, 3, 7, 27))]
        for k, dtype in enumerate((Z.T_UINT, Z.T_F32, Z.T_F16, Z.T_BF16)):
            E._check(images, (9 + k, 66 - Cn), dtype, "chw" if (k + Cn) %% 2 else "hwc", bool((k + P // 8) %% 2), scale=E.SCALE, bias=E.BIAS,
                     tile=(64 - 9 * k, 5), grid=k)
E._check([(E._img(rng, 7, 192, 4, 16), None)], (5, 3), Z.T_F32, "chw", True)
E._check([(E._img(rng, 128, 50, 4, 8), None)], (2, 70), Z.T_UINT, "hwc", True)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_RESIZE_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
