"""The general PNG de-filter kernel (csrc/png_spec_kernel.inc) on the CPU lock-step emulator, under ASan/UBSan, against
the reference decoder of tests/png_spec_ref.py: every filter unit, every filter type, widths 1..130 (sub-byte row tails,
empty Adam7 passes), heights across band edges."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402
from emu_binding import load_emu  # noqa: E402


class SpecTask(C.Structure):  # include/debig_hip.h: debig_png_spec_task
    _fields_ = [("stream_off", C.c_uint64), ("rgba_off", C.c_uint64), ("pal_off", C.c_uint64), ("scratch_off", C.c_uint64),
                ("width", C.c_uint32), ("height", C.c_uint32), ("img_width", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32),
                ("bpp_f", C.c_uint8), ("depth", C.c_uint8), ("color_type", C.c_uint8), ("channels", C.c_uint8),
                ("key", C.c_uint16 * 3), ("has_key", C.c_uint16), ("n_pal", C.c_uint16), ("reserved16", C.c_uint16),
                ("reserved", C.c_uint32)]


class SpecResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("bad_row", C.c_uint32)]


def _a16(x):
    return (x + 15) // 16 * 16


_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_SPEC_EMU_ASAN") == "1")
        L.emu_png_spec_defilter_batch.restype = C.c_int
        L.emu_png_spec_defilter_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def run_images(imgs):
    """imgs: [dict(samples, ct, depth, interlace, filters, key, pal (n, 3), trns)] -> [(status list, rgba)]"""
    arena = bytearray(64)
    tasks, owners, rgba_offs = [], [], []
    rgba_total = 0
    for i, im in enumerate(imgs):
        s = im["samples"]
        h, w = s.shape[:2]
        ct, depth, il = im["ct"], im["depth"], im.get("interlace", 0)
        stream = R.scanlines(s, ct, depth, il, im.get("filters"))
        pal_off = 0
        if ct == 3:
            pal_off = len(arena)
            arena += R.full_palette(im["pal"], im.get("trns", b"")).tobytes()
        base = len(arena)
        arena += stream + bytes(_a16(len(stream)) - len(stream) + 32)
        rgba_offs.append(rgba_total)
        pos = 0
        for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
            rb = R.row_bytes(wp, ct, depth)
            t = SpecTask()
            t.stream_off, t.rgba_off, t.pal_off = base + pos, rgba_total, pal_off
            t.width, t.height, t.img_width = wp, hp, w
            t.x0, t.y0, t.dx, t.dy = x0, y0, dx, dy
            t.bpp_f, t.depth, t.color_type, t.channels = R.bpp_f(ct, depth), depth, ct, R.CHANNELS[ct]
            key = im.get("key")
            if key is not None:
                t.has_key = 1
                for k, v in enumerate(key):
                    t.key[k] = v
            t.n_pal = len(im["pal"]) if ct == 3 else 0
            tasks.append(t)
            owners.append(i)
            pos += hp * (1 + rb)
        rgba_total += _a16(4 * w * h) + 16
    for t in tasks:  # scratch rings after everything
        rb = R.row_bytes(t.width, t.color_type, t.depth)
        arena += bytes(_a16(len(arena)) - len(arena))
        t.scratch_off = len(arena)
        arena += bytes(4 * (_a16(rb) + 16))
    arena += bytes(64)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    rgba = np.full(rgba_total + 64, 0xEE, dtype=np.uint8)
    n = len(tasks)
    T = (SpecTask * n)(*tasks)
    res = (SpecResult * n)()
    assert _emu().emu_png_spec_defilter_batch(a.ctypes.data, rgba.ctypes.data, T, res, n) == 0
    out = []
    for i, im in enumerate(imgs):
        h, w = im["samples"].shape[:2]
        st = [(res[k].status, res[k].bad_row) for k in range(n) if owners[k] == i]
        out.append((st, rgba[rgba_offs[i]: rgba_offs[i] + 4 * w * h].reshape(h, w, 4)))
    return out


def expected(im):
    ct, depth = im["ct"], im["depth"]
    pal = None
    if ct == 3:
        pal = [tuple(int(v) for v in p) for p in im["pal"]]
    trns = im.get("trns")
    if im.get("key") is not None:
        trns = np.asarray(im["key"], dtype=">u2").tobytes()
    png = R.encode(im["samples"], ct, depth, im.get("interlace", 0), trns=trns, palette=pal, filters=im.get("filters"))
    st, px, _ = R.decode(png)
    assert st == R.OK, st
    return px


def _image(rng, w, h, ct, depth, interlace=0, filters=None, key=False):
    im = dict(ct=ct, depth=depth, interlace=interlace, filters=filters)
    if ct == 3:
        n_pal = int(rng.integers(1, (1 << depth) + 1))
        im["pal"] = rng.integers(0, 256, size=(n_pal, 3))
        im["trns"] = bytes(rng.integers(0, 256, size=int(rng.integers(0, n_pal + 1))).astype(np.uint8))
        im["samples"] = R.random_image(rng, w, h, ct, depth, n_pal)
    else:
        # few distinct values so that the tRNS key matches somewhere
        s = R.random_image(rng, w, h, ct, depth)
        if key:
            s = s % 3 if depth != 16 else (s % 3) * 257
            im["key"] = tuple(int(v) for v in s[0, 0][: 3 if ct == 2 else 1])
        im["samples"] = s
    return im


FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16),
           (6, 8), (6, 16)]


def _check(imgs):
    for im, (st, px) in zip(imgs, run_images(imgs)):
        assert all(s == (0, 0xFFFFFFFF) for s in st), (im["ct"], im["depth"], im["samples"].shape, st)
        exp = expected(im)
        assert np.array_equal(px, exp), (im["ct"], im["depth"], im["samples"].shape, im.get("interlace"),
                                         np.argwhere(px != exp)[:4])


@pytest.mark.parametrize("ct,depth", FORMATS)
def test_every_unit_and_filter_type(ct, depth):
    """every filter type on its own, and mixed per row, interlaced and not, with tRNS where it applies"""
    rng = np.random.default_rng(ct * 100 + depth)
    imgs = []
    for ft in range(5):
        imgs.append(_image(rng, 37, 9, ct, depth, 0, ft, key=ct in (0, 2)))
    imgs.append(_image(rng, 29, 23, ct, depth, 1, None, key=ct in (0, 2)))
    _check(imgs)


@pytest.mark.parametrize("ct,depth", [(0, 1), (0, 2), (0, 4), (3, 4), (2, 16), (6, 16), (4, 8), (6, 8)])
def test_widths_1_to_130(ct, depth):
    """every width 1..130 (sub-byte row tails; Adam7 passes that are empty for w or h < 5)"""
    rng = np.random.default_rng(7 + depth)
    imgs = [_image(rng, w, 1 + (w % 7), ct, depth, w % 2, None) for w in range(1, 131)]
    _check(imgs)


@pytest.mark.parametrize("h", [63, 64, 65, 129])
def test_heights_across_bands(h):
    """bands of 64 rows handed from wavefront to wavefront through the scratch ring"""
    rng = np.random.default_rng(h)
    imgs = [_image(rng, 45, h, 6, 16, 0, None), _image(rng, 70, h, 0, 1, 0, 4), _image(rng, 33, h, 2, 8, 1, None),
            _image(rng, 19, h, 3, 8, 0, 3)]
    _check(imgs)


def test_bad_filter_byte_and_palette_index():
    rng = np.random.default_rng(5)
    good = _image(rng, 40, 70, 6, 8, 0, None)
    bad_ft = _image(rng, 40, 70, 0, 8, 0, lambda p, y: 5 if y == 66 else 1)
    pal = _image(rng, 40, 70, 3, 8, 0, None)
    pal["pal"] = pal["pal"][:3]
    pal["samples"][30, 7] = 200  # index past the 3 entries
    res = run_images([good, bad_ft, pal])
    assert res[0][0] == [(0, 0xFFFFFFFF)]
    assert res[1][0][0] == (1, 66)
    assert res[2][0][0][0] == 2
    assert np.array_equal(res[0][1], expected(good))


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so): every filter unit, interlaced and
    not, narrow and across a band edge.  Runs in a child process (the sanitizer runtime has to be loaded first)."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_png_spec as T
rng = np.random.default_rng(11)
imgs = [T._image(rng, w, h, ct, d, il, None, key=ct in (0, 2))
        for (ct, d) in T.FORMATS for (w, h, il) in ((1, 1, 0), (3, 2, 1), (13, 66, 0), (9, 7, 1))]
T._check(imgs)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_SPEC_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
