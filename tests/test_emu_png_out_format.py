"""The output-format twin of the general PNG de-filter (csrc/png_spec_kernel.inc: debig_png_spec_defilter_fmt_kernel) on
the CPU lock-step emulator, plain and under ASan/UBSan, against the numpy converter of tests/png_out_format_ref.py:
every filter unit x every filter type x every output format x interlace 0/1, widths 1..70, heights across the 64-row
band edges and past the wrap of the scratch ring (4, 5 and 6 bands, every filter unit), rows of 8 to 72 groups of filter unit 6
across three bands, short palettes and tRNS keys; with out_fmt = 0 it must equal debig_png_spec_defilter_kernel byte for byte.
Every byte between and after the images must stay untouched, and every byte of the arena outside the scratch rings.  run_images
launches through the seam tests/stage_launch.py: tests/test_gpu_png_defilter_kernels.py runs the same cases on the GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_out_format_ref as F  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_emu_png_spec as T  # noqa: E402
from emu_binding import load_emu  # noqa: E402


class SpecTask(C.Structure):  # include/debig_hip.h: debig_png_spec_task (reserved16 is now out_fmt)
    _fields_ = [("stream_off", C.c_uint64), ("rgba_off", C.c_uint64), ("pal_off", C.c_uint64), ("scratch_off", C.c_uint64),
                ("width", C.c_uint32), ("height", C.c_uint32), ("img_width", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("dx", C.c_uint32), ("dy", C.c_uint32),
                ("bpp_f", C.c_uint8), ("depth", C.c_uint8), ("color_type", C.c_uint8), ("channels", C.c_uint8),
                ("key", C.c_uint16 * 3), ("has_key", C.c_uint16), ("n_pal", C.c_uint16), ("out_fmt", C.c_uint16),
                ("reserved", C.c_uint32)]


assert C.sizeof(SpecTask) == C.sizeof(T.SpecTask) == 80
assert SpecTask.out_fmt.offset == T.SpecTask.reserved16.offset

CONCRETE = [lay | d for d in (F.D8, F.D16) for lay in (F.RGBA, F.RGB, F.GRAY, F.GRAY_ALPHA)]
_LIB = {}
FILL = 0xEE


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_SPEC_EMU_ASAN") == "1")
        L.emu_png_spec_defilter_fmt_batch.restype = C.c_int
        L.emu_png_spec_defilter_fmt_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


def _has_trns(im):
    return int(im.get("key") is not None) if im["ct"] in (0, 2) else int(im["ct"] == 3 and len(im.get("trns", b"")) > 0)


def run_images(imgs, fmts):
    """imgs as test_emu_png_spec._image makes them, fmts: one out_format per image (NATIVE resolved here as the host
    does) -> [(status list, pixels (h, w, channels), resolved format)]; asserts that no byte outside the images changed"""
    arena = bytearray(64)
    tasks, owners, offs, sizes, res_fmts = [], [], [], [], []
    total = 0
    for i, (im, fmt) in enumerate(zip(imgs, fmts)):
        s = im["samples"]
        h, w = s.shape[:2]
        ct, depth, il = im["ct"], im["depth"], im.get("interlace", 0)
        lay, bits = F.resolve(ct, depth, _has_trns(im), fmt)
        rf = lay | (F.D16 if bits == 16 else F.D8)
        res_fmts.append(rf)
        nbytes = w * h * F.LAYOUT_CHANNELS[lay] * bits // 8
        stream = R.scanlines(s, ct, depth, il, im.get("filters"))
        pal_off = 0
        if ct == 3:
            pal_off = len(arena)
            arena += R.full_palette(im["pal"], im.get("trns", b"")).tobytes()
        base = len(arena)
        arena += stream + bytes(T._a16(len(stream)) - len(stream) + 32)
        offs.append(total)
        sizes.append(nbytes)
        pos = 0
        for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
            t = SpecTask()
            t.stream_off, t.rgba_off, t.pal_off = base + pos, total, pal_off
            t.width, t.height, t.img_width = wp, hp, w
            t.x0, t.y0, t.dx, t.dy = x0, y0, dx, dy
            t.bpp_f, t.depth, t.color_type, t.channels = R.bpp_f(ct, depth), depth, ct, R.CHANNELS[ct]
            if im.get("key") is not None:
                t.has_key = 1
                for k, v in enumerate(im["key"]):
                    t.key[k] = v
            t.n_pal = len(im["pal"]) if ct == 3 else 0
            t.out_fmt = rf
            tasks.append(t)
            owners.append(i)
            pos += hp * (1 + R.row_bytes(wp, ct, depth))
        total += T._a16(nbytes) + 16
    for t in tasks:
        rb = R.row_bytes(t.width, t.color_type, t.depth)
        arena += bytes(T._a16(len(arena)) - len(arena))
        t.scratch_off = len(arena)
        arena += bytes(4 * (T._a16(rb) + 16))
    arena += bytes(64)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    out = np.full(total + 64, FILL, dtype=np.uint8)
    n = len(tasks)
    TT = (SpecTask * n)(*tasks)
    res = (T.SpecResult * n)()
    T.launch_defilter("png_spec_defilter_fmt", a, out, TT, res, _emu)
    T.assert_fill_outside(out, zip(offs, sizes), FILL)
    result = []
    for i, im in enumerate(imgs):
        h, w = im["samples"].shape[:2]
        lay, bits = res_fmts[i] & 15, 16 if res_fmts[i] & F.D16 else 8
        st = [(res[k].status, res[k].bad_row) for k in range(n) if owners[k] == i]
        px = out[offs[i]: offs[i] + sizes[i]].view("<u2" if bits == 16 else np.uint8).reshape(h, w, F.LAYOUT_CHANNELS[lay])
        result.append((st, px, res_fmts[i]))
    return result


def expected(im, fmt):
    ct, depth = im["ct"], im["depth"]
    pal = R.full_palette(im["pal"], im.get("trns", b""))[: len(im["pal"])] if ct == 3 else None
    s = im["samples"]
    if s.ndim == 2:
        s = s[:, :, None]
    return F.convert(s, ct, depth, im.get("key"), pal, fmt, has_trns=_has_trns(im))


def _check(imgs, fmts):
    for im, fmt, (st, px, rf) in zip(imgs, fmts, run_images(imgs, fmts)):
        where = (im["ct"], im["depth"], im["samples"].shape, im.get("interlace"), hex(fmt))
        assert all(s == (0, 0xFFFFFFFF) for s in st), (where, st)
        exp = expected(im, fmt)
        assert px.shape == exp.shape, where
        assert np.array_equal(px, exp), (where, np.argwhere(px != exp)[:4])


ALL_FMTS = CONCRETE + [F.NATIVE, F.NATIVE | F.D16, F.NATIVE | F.D_NATIVE]


@pytest.mark.parametrize("ct,depth", T.FORMATS)
def test_every_unit_filter_type_and_format(ct, depth):
    """every filter type on its own and mixed per row, interlaced and not, tRNS keys, to every output format (every
    format in one launch: out_fmt is per task)"""
    rng = np.random.default_rng(ct * 100 + depth + 1)
    imgs, fmts = [], []
    for k, fmt in enumerate(ALL_FMTS):
        for ft in range(5):
            imgs.append(T._image(rng, 21 + k, 9, ct, depth, 0, ft, key=ct in (0, 2) and (k + ft) % 2 == 0))
            fmts.append(fmt)
        imgs.append(T._image(rng, 19 + k, 17, ct, depth, 1, None, key=ct in (0, 2) and k % 2 == 0))
        fmts.append(fmt)
    _check(imgs, fmts)


@pytest.mark.parametrize("ct,depth", [(0, 1), (0, 2), (0, 4), (3, 1), (3, 4), (2, 16), (6, 16), (4, 8), (2, 8), (0, 16)])
def test_widths_1_to_70(ct, depth):
    """every width 1..70 (sub-byte row tails, partial groups, empty Adam7 passes), formats in rotation"""
    rng = np.random.default_rng(17 + depth * 10 + ct)
    imgs = [T._image(rng, w, 1 + (w % 7), ct, depth, w % 2, None, key=ct in (0, 2) and w % 3 == 0) for w in range(1, 71)]
    fmts = [ALL_FMTS[w % len(ALL_FMTS)] for w in range(1, 71)]
    _check(imgs, fmts)


@pytest.mark.parametrize("h", [63, 64, 65, 129])
def test_heights_across_bands(h):
    rng = np.random.default_rng(h + 1)
    imgs = [T._image(rng, 45, h, 6, 16, 0, None), T._image(rng, 70, h, 0, 1, 0, 4), T._image(rng, 33, h, 2, 8, 1, None),
            T._image(rng, 19, h, 3, 8, 0, 3), T._image(rng, 27, h, 4, 16, 1, None)]
    for fmts in ([F.GRAY | F.D16] * 5, [F.RGB, F.GRAY_ALPHA, F.NATIVE | F.D_NATIVE, F.RGBA | F.D16, F.GRAY]):
        _check(imgs, fmts)


@pytest.mark.parametrize("ct,depth", T.UNIT_FORMATS)
@pytest.mark.parametrize("h", T.WRAP_HEIGHTS)
def test_heights_past_the_ring_wrap(h, ct, depth):
    """four, five and six bands (test_emu_png_spec.wrap_images), output formats in rotation"""
    imgs = T.wrap_images(np.random.default_rng(h * 100 + ct * 10 + depth + 1), h, ct, depth)
    k0 = h + T.UNIT_FORMATS.index((ct, depth))
    _check(imgs, [ALL_FMTS[(k0 + k) % len(ALL_FMTS)] for k in range(len(imgs))])


@pytest.mark.parametrize("ng", T.LONG_NGROUPS)
def test_long_rows_across_bands(ng):
    """filter unit 6: rows of 8 to 72 groups over three bands (test_emu_png_spec.long_image), Paeth throughout"""
    _check([T.long_image(np.random.default_rng(ng + 1), 2, 16, ng)], [ALL_FMTS[ng % len(ALL_FMTS)]])


def test_short_palette_and_keys():
    """a palette of fewer than 256 entries with a shorter tRNS (uncovered entries 255), 8- and 16-bit keys"""
    rng = np.random.default_rng(21)
    imgs, fmts = [], []
    for fmt in ALL_FMTS:
        p = T._image(rng, 23, 11, 3, 8, 0, None)
        p["pal"] = p["pal"][:5] if len(p["pal"]) > 5 else p["pal"]
        p["samples"] = (p["samples"] % len(p["pal"])).astype(np.uint8)
        p["trns"] = bytes([0, 128, 7])[: len(p["pal"]) - 1]
        imgs += [p, T._image(rng, 23, 11, 0, 16, 1, None, key=True), T._image(rng, 23, 11, 2, 16, 0, 2, key=True),
                 T._image(rng, 23, 11, 0, 2, 0, 1, key=True)]
        fmts += [fmt] * 4
    _check(imgs, fmts)


def test_format_zero_equals_the_rgba8_kernel():
    rng = np.random.default_rng(23)
    imgs = [T._image(rng, w, h, ct, d, il, None, key=ct in (0, 2))
            for (ct, d) in T.FORMATS for (w, h, il) in ((1, 1, 0), (7, 5, 1), (37, 66, 0), (30, 13, 1))]
    old = T.run_images(imgs)
    new = run_images(imgs, [0] * len(imgs))
    for im, (st0, px0), (st1, px1, rf) in zip(imgs, old, new):
        assert rf == 0 and st0 == st1
        assert px1.dtype == np.uint8 and px0.tobytes() == px1.tobytes(), (im["ct"], im["depth"])


def test_errors_under_a_format():
    """the filter-byte and palette-index statuses of the twin kernel are those of the RGBA8 kernel"""
    rng = np.random.default_rng(5)
    good = T._image(rng, 40, 70, 6, 8, 0, None)
    bad_ft = T._image(rng, 40, 70, 0, 8, 0, lambda p, y: 5 if y == 66 else 1)
    pal = T._image(rng, 40, 70, 3, 8, 0, None)
    pal["pal"] = pal["pal"][:3]
    pal["samples"][30, 7] = 200
    res = run_images([good, bad_ft, pal], [F.GRAY | F.D16, F.RGB, F.NATIVE])
    assert res[0][0] == [(0, 0xFFFFFFFF)]
    assert res[1][0][0] == (1, 66)
    assert res[2][0][0][0] == 2
    assert np.array_equal(res[0][1], expected(good, F.GRAY | F.D16))


def test_kernel_under_address_sanitizer():
    """the same kernel source under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_png_out_format as E
import test_emu_png_spec as T
rng = np.random.default_rng(13)
imgs, fmts = [], []
for k, (ct, d) in enumerate(T.FORMATS):
    for j, (w, h, il) in enumerate(((1, 1, 0), (3, 2, 1), (13, 66, 0), (9, 7, 1), (17, 3, 0))):
        imgs.append(T._image(rng, w, h, ct, d, il, None, key=ct in (0, 2)))
        fmts.append(E.ALL_FMTS[(k + j) %% len(E.ALL_FMTS)])
E._check(imgs, fmts)
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_SPEC_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
