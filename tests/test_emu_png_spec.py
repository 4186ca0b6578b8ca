"""The general PNG de-filter kernel (csrc/png_spec_kernel.inc) on the CPU lock-step emulator, under ASan/UBSan, against
the reference decoder of tests/png_spec_ref.py: every filter unit, every filter type, widths 1..130 (sub-byte row tails,
empty Adam7 passes), heights across band edges and past the wrap of the four-row scratch ring (4, 5 and 6 bands), rows of 8 to 72
groups across three bands, scanline bytes at every residue mod 4.  run_images launches through the seam tests/stage_launch.py, so
tests/test_gpu_png_defilter_kernels.py runs the same cases on the GPU; on either back end the arena outside the scratch rings and
the output arena outside the images must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402


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


def launch_defilter(name, a, out, tasks, res, emu):
    """one launch of a general de-filter kernel through the launch seam (tests/stage_launch.py: the emulator, or the product library
    on the GPU) on the arena a, the output arena out, the ctypes task and result arrays.  The kernel may write into the arena only
    inside the tasks' scratch rings, [scratch_off, scratch_off + 4 * (a16(row bytes) + 16)) as the runners allocate them: every other
    byte of it -- streams, palettes, padding -- must come back as it went in."""
    before = a.copy()
    assert a.ctypes.data % 4 == 0 and out.ctypes.data % 4 == 0  # (an offset's residue mod 4 is its address's: the kernel works in dwords)
    assert launch(name, a, out, tasks, res, len(tasks), 0, emu=emu) == 0
    fixed = np.ones(len(a), dtype=bool)
    for t in tasks:
        fixed[t.scratch_off: t.scratch_off + 4 * (_a16(R.row_bytes(t.width, t.color_type, t.depth)) + 16)] = False
    assert np.array_equal(a[fixed], before[fixed]), ("the arena was written outside the scratch rings", np.flatnonzero((a != before) & fixed)[:8])


def assert_fill_outside(out, spans, fill):
    """every byte of the output arena outside the images' (offset, size) spans -- the 16-byte gaps, the tail -- keeps its fill"""
    untouched = np.ones(len(out), dtype=bool)
    for off, size in spans:
        untouched[off: off + size] = False
    assert (out[untouched] == fill).all(), ("bytes outside the images were written", np.flatnonzero(untouched & (out != fill))[:8])


def run_images(imgs, shift=0, placed=None):
    """imgs: [dict(samples, ct, depth, interlace, filters, key, pal (n, 3), trns)] -> [(status list, rgba)].  shift: every image's
    scanline bytes start this many bytes behind a multiple of 16; placed: a list that receives every task's stream_off"""
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
        arena += bytes(shift)
        base = len(arena)
        arena += stream + bytes(_a16(shift + len(stream)) - shift - len(stream) + 32)
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
    launch_defilter("png_spec_defilter", a, rgba, T, res, _emu)
    assert_fill_outside(rgba, [(rgba_offs[i], 4 * im["samples"].shape[0] * im["samples"].shape[1]) for i, im in enumerate(imgs)], 0xEE)
    if placed is not None:
        placed.extend(t.stream_off for t in tasks)
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


def _check(imgs, **kw):
    for im, (st, px) in zip(imgs, run_images(imgs, **kw)):
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


# ---- past the ring wrap, long rows, stream alignment: the shapes at which the hand-over between the wavefronts can go wrong ----------
# (shared with the batteries of the other three store stages: tests/test_emu_png_out_format.py, _planar.py, _labels.py)

GROUP_BYTES = {1: 8, 2: 8, 3: 12, 4: 16, 6: 12, 8: 16}  # filter unit -> bytes per group (png_spec_kernel.inc: PngSpecShape<BPP>::GB)
# every filter unit the kernel is instantiated for: 1 (sub-byte and 8-bit), 2, 3, 4, 6, 8
UNIT_FORMATS = [(0, 1), (0, 4), (3, 8), (0, 16), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16)]
WRAP_HEIGHTS = [256, 257, 321]  # 4, 5 and 6 bands of 64 rows: bands 4 and 5 take the ring rows of bands 0 and 1 (PNG_SPEC_NWD = 4)
LONG_FORMATS = [(0, 4), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16)]  # one format per filter unit
LONG_NGROUPS = [8, 9, 63, 64, 65, 72]  # on both sides of PNG_SPEC_BLOCK = 8 and of the 63 steps that lane 63 runs behind lane 0


def ngroups(w, ct, depth):
    return -(-R.row_bytes(w, ct, depth) // GROUP_BYTES[R.bpp_f(ct, depth)])


def _widest(ct, depth, rb):
    """the widest row of at most rb bytes"""
    return rb * 8 // (R.CHANNELS[ct] * depth)


def wrap_images(rng, h, ct, depth):
    """images of h rows whose rows are one group and three groups long, each also with a partial last group (sub-byte samples:
    with a partial last byte too), under filter 4, 3 and 2 on every row and under the default mix, so that every band edge is crossed
    by each filter that reads the row above; for sub-byte samples also an Adam7 image whose seventh pass has h + 1 rows"""
    unit = R.bpp_f(ct, depth)
    gb = GROUP_BYTES[unit]
    sub = int(depth < 8)
    full1, part1 = _widest(ct, depth, gb), _widest(ct, depth, gb - unit) - sub
    full3, part3 = _widest(ct, depth, 3 * gb), _widest(ct, depth, 3 * gb - unit) - sub
    assert [ngroups(w, ct, depth) for w in (full1, part1, full3, part3)] == [1, 1, 3, 3]
    assert R.row_bytes(full1, ct, depth) == gb and R.row_bytes(full3, ct, depth) == 3 * gb
    assert R.row_bytes(part1, ct, depth) % gb and R.row_bytes(part3, ct, depth) % gb and -(-h // 64) >= 4
    imgs = [_image(rng, w, h, ct, depth, 0, ft)
            for ft, ws in ((4, (full1, part3)), (3, (part1, full3)), (2, (full1, part3)), (None, (part1, full3))) for w in ws]
    if sub:
        imgs.append(_image(rng, 11, 2 * h + 3, ct, depth, 1, None))
        assert R.passes(11, 2 * h + 3, 1)[6][5] == h + 1 > 256
    return imgs


def long_image(rng, ct, depth, ng):
    """130 rows (three bands) of ng groups, the last one partial where ng is odd, Paeth on every row: one wrong "up" byte at a band
    edge propagates to the end of the image"""
    unit = R.bpp_f(ct, depth)
    w = _widest(ct, depth, ng * GROUP_BYTES[unit] - (unit if ng % 2 else 0))
    assert ngroups(w, ct, depth) == ng
    return _image(rng, w, 130, ct, depth, 0, 4)


@pytest.mark.parametrize("ct,depth", UNIT_FORMATS)
@pytest.mark.parametrize("h", WRAP_HEIGHTS)
def test_heights_past_the_ring_wrap(h, ct, depth):
    """four, five and six bands: the fifth and sixth band's last rows go where the first and second band's were"""
    _check(wrap_images(np.random.default_rng(h * 100 + ct * 10 + depth), h, ct, depth))


@pytest.mark.parametrize("ng", LONG_NGROUPS)
@pytest.mark.parametrize("ct,depth", LONG_FORMATS)
def test_long_rows_across_bands(ct, depth, ng):
    """rows longer than one load phase: the wavefront of the band below waits in mid-row for the groups it needs next"""
    _check([long_image(np.random.default_rng(ng * 100 + ct * 10 + depth), ct, depth, ng)])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_stream_alignment(shift):
    """the same two-band images of the filter units 1, 3 and 6 with their scanline bytes at every residue mod 4"""
    rng = np.random.default_rng(31)
    imgs = [_image(rng, 21, 66, ct, depth, 0, ft) for ct, depth in ((0, 2), (2, 8), (2, 16)) for ft in (None, 4)]
    placed = []
    _check(imgs, shift=shift, placed=placed)
    assert len(placed) == len(imgs) and all(p & 3 == shift for p in placed), placed


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
