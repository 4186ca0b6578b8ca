"""The two kernels of debig_png_decode_batch_labels on the CPU lock-step emulator, against tests/png_label_ref.py:
  * debig_png_spec_defilter_index_kernel (csrc/png_spec_kernel.inc): colour type 0 at depths 1, 2, 4, 8, 16 and colour type 3
    at 1, 2, 4, 8, plain and Adam7, sizes from 1 x 1 (most Adam7 passes empty) to 3 x 130 (three 64-row bands), row filters
    cycling y % 5, then 4, 5 and 6 bands (the four-row scratch ring wraps) and rows of 8 to 72 groups across three bands; the bytes
    are labels(), every byte beyond the images keeps its sentinel and every byte of the arena outside the scratch rings its value; an
    index >= n_pal fails the task; run_index launches through the seam, and tests/test_gpu_png_defilter_kernels.py runs it on the GPU;
  * debig_png_label_gather_kernel (csrc/png_label_kernel.inc): 1- and 2-byte sources into all four dtypes, output widths that
    are no multiple of any per-lane count, boxes at each corner, a 1-pixel-wide box, enlarging 40 x, with and without a LUT,
    a 4 KiB sentinel kept before and after the tensor; tasks that break a bound are skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_emu_png_spec as T  # noqa: E402
from emu_binding import load_emu  # noqa: E402
from stage_launch import launch  # noqa: E402

FILL = 0xEE
LABEL_FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (3, 1), (3, 2), (3, 4), (3, 8)]
SIZES = [(1, 1), (7, 3), (9, 9), (45, 70), (3, 130)]  # (w, h)


class LabelTask(C.Structure):  # include/debig_hip.h: debig_png_label_task
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("sx_off", C.c_uint64), ("sy_off", C.c_uint64),
                ("src_pitch", C.c_uint32), ("out_w", C.c_uint32), ("out_h", C.c_uint32), ("row0", C.c_uint32), ("rows", C.c_uint32),
                ("src_bytes", C.c_uint8), ("dtype", C.c_uint8), ("reserved", C.c_uint16)]


assert C.sizeof(LabelTask) == 56
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu(asan=os.environ.get("DEBIG_SPEC_EMU_ASAN") == "1")
        L.emu_png_spec_defilter_index_batch.restype = C.c_int
        L.emu_png_spec_defilter_index_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.emu_png_label_gather_batch.restype = C.c_int
        L.emu_png_label_gather_batch.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


# ---- the index de-filter ------------------------------------------------------------------------------------------------------

def run_index(imgs):
    """imgs as test_emu_png_spec._image makes them -> [(status list, labels (h, w) uint8 / uint16)]; asserts that no byte
    outside the images changed"""
    arena = bytearray(64)
    tasks, owners, offs, sizes = [], [], [], []
    total = 0
    for i, im in enumerate(imgs):
        s = im["samples"]
        h, w = s.shape[:2]
        ct, depth, il = im["ct"], im["depth"], im.get("interlace", 0)
        es = 2 if depth == 16 else 1
        stream = R.scanlines(s, ct, depth, il, im.get("filters"))
        base = len(arena)
        arena += stream + bytes(T._a16(len(stream)) - len(stream) + 32)
        offs.append(total)
        sizes.append(w * h * es)
        pos = 0
        for x0, y0, dx, dy, wp, hp in R.passes(w, h, il):
            t = T.SpecTask()
            t.stream_off, t.rgba_off, t.pal_off = base + pos, total, 0  # (no palette in the arena: the kernel must not read one)
            t.width, t.height, t.img_width = wp, hp, w
            t.x0, t.y0, t.dx, t.dy = x0, y0, dx, dy
            t.bpp_f, t.depth, t.color_type, t.channels = R.bpp_f(ct, depth), depth, ct, R.CHANNELS[ct]
            t.n_pal = len(im["pal"]) if ct == 3 else 0
            tasks.append(t)
            owners.append(i)
            pos += hp * (1 + R.row_bytes(wp, ct, depth))
        total += T._a16(w * h * es) + 16
    for t in tasks:
        rb = R.row_bytes(t.width, t.color_type, t.depth)
        arena += bytes(T._a16(len(arena)) - len(arena))
        t.scratch_off = len(arena)
        arena += bytes(4 * (T._a16(rb) + 16))
    arena += bytes(64)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    out = np.full(total + 64, FILL, dtype=np.uint8)
    n = len(tasks)
    TT = (T.SpecTask * n)(*tasks)
    res = (T.SpecResult * n)()
    T.launch_defilter("png_spec_defilter_index", a, out, TT, res, _emu)
    untouched = np.ones(len(out), dtype=bool)
    result = []
    for i, im in enumerate(imgs):
        h, w = im["samples"].shape[:2]
        untouched[offs[i]: offs[i] + sizes[i]] = False
        st = [(res[k].status, res[k].bad_row) for k in range(n) if owners[k] == i]
        result.append((st, out[offs[i]: offs[i] + sizes[i]].view("<u2" if im["depth"] == 16 else np.uint8).reshape(h, w)))
    assert (out[untouched] == FILL).all(), "bytes outside the images were written"
    return result


def _png(im):
    pal = [tuple(int(v) for v in p) for p in im["pal"]] if im["ct"] == 3 else None
    return R.encode(im["samples"], im["ct"], im["depth"], im.get("interlace", 0), palette=pal, filters=im.get("filters"))


def _index_images(seed, formats=LABEL_FORMATS, sizes=SIZES):
    rng = np.random.default_rng(seed)
    return [T._image(rng, w, h, ct, depth, il, lambda p, y: y % 5)
            for ct, depth in formats for w, h in sizes for il in (0, 1)]


def _check_index(imgs):
    for im, (st, lab) in zip(imgs, run_index(imgs)):
        where = (im["ct"], im["depth"], im["samples"].shape, im.get("interlace"))
        assert all(s == (0, 0xFFFFFFFF) for s in st), (where, st)
        est, exp, _ = LR.labels(_png(im))
        assert est == R.OK, where
        assert lab.shape == exp.shape and np.array_equal(lab, exp), (where, np.argwhere(lab != exp)[:4])


@pytest.mark.parametrize("ct,depth", LABEL_FORMATS)
def test_index_defilter_every_label_format(ct, depth):
    _check_index(_index_images(ct * 100 + depth, [(ct, depth)]))


def test_index_defilter_every_filter_type_and_widths_1_to_70():
    """every filter type on its own over a band edge, and every width 1 .. 70 (sub-byte row tails, partial groups)"""
    rng = np.random.default_rng(8)
    imgs = [T._image(rng, 37, 66, ct, depth, 0, ft) for ct, depth in ((0, 2), (3, 8), (0, 16)) for ft in range(5)]
    imgs += [T._image(rng, w, 1 + w % 5, *LABEL_FORMATS[w % len(LABEL_FORMATS)], w % 2, None) for w in range(1, 71)]
    _check_index(imgs)


@pytest.mark.parametrize("ct,depth", [f for f in T.UNIT_FORMATS if f in LABEL_FORMATS])
@pytest.mark.parametrize("h", T.WRAP_HEIGHTS)
def test_heights_past_the_ring_wrap(h, ct, depth):
    """four, five and six bands (test_emu_png_spec.wrap_images) in the label formats of both filter units of this kernel, 1 and 2"""
    assert T.R.bpp_f(ct, depth) == (2 if depth == 16 else 1)
    _check_index(T.wrap_images(np.random.default_rng(h * 100 + ct * 10 + depth + 3), h, ct, depth))


@pytest.mark.parametrize("ng", T.LONG_NGROUPS)
def test_long_rows_across_bands(ng):
    """filter unit 2: rows of 8 to 72 groups over three bands (test_emu_png_spec.long_image), Paeth throughout"""
    _check_index([T.long_image(np.random.default_rng(ng + 3), 0, 16, ng)])


def test_index_past_the_palette_and_other_colour_types_fail_the_task():
    rng = np.random.default_rng(5)
    good = T._image(rng, 40, 70, 3, 8, 0, None)
    good["samples"] = (good["samples"] % len(good["pal"])).astype(np.uint8)
    pal = T._image(rng, 40, 70, 3, 8, 0, None)
    pal["pal"] = pal["pal"][:3]
    pal["samples"][30, 7] = 200  # index past the 3 entries
    sub = T._image(rng, 21, 9, 3, 2, 1, None)
    sub["pal"] = sub["pal"][:2]
    sub["samples"][:] = 0
    sub["samples"][8, 20] = 2  # the last pixel of the last row: inside the image, past the palette
    tail = T._image(rng, 21, 9, 3, 2, 0, None)
    tail["pal"] = tail["pal"][:1]
    tail["samples"][:] = 0
    bad_ft = T._image(rng, 40, 70, 0, 8, 0, lambda p, y: 5 if y == 66 else 1)
    rgb = T._image(rng, 8, 8, 2, 8, 0, None)
    ga = T._image(rng, 8, 8, 4, 8, 0, None)
    res = run_index([good, pal, sub, tail, bad_ft, rgb, ga])
    assert res[0][0] == [(0, 0xFFFFFFFF)] and np.array_equal(res[0][1], good["samples"][:, :, 0])
    assert res[1][0][0][0] == 2
    assert 2 in [s for s, _ in res[2][0]]
    assert res[3][0] == [(0, 0xFFFFFFFF)]
    assert res[4][0][0] == (1, 66)
    assert res[5][0][0][0] == 1 and res[6][0][0][0] == 1  # not label tasks: the internal guard
    assert (res[5][1] == FILL).all() and (res[6][1] == FILL).all()


# ---- the gather --------------------------------------------------------------------------------------------------------------

def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off: off + nbytes]


def run_gather(srcs, jobs, size, dtype, lut=None, run=None, grid=0):
    """srcs: [(h, w) uint8 / uint16 label arrays]; jobs: [(source index, box or None)] -> (len(jobs), H, W) of dtype.  The
    tables and tasks are made as the host makes them (run: output rows per task, default the host's 16384 elements)"""
    H, W = size
    es = np.dtype(LR.DTYPES[dtype]).itemsize
    arena, soff = bytearray(16), []
    for s in srcs:
        arena += bytes(-len(arena) % 16)
        soff.append(len(arena))
        arena += np.ascontiguousarray(s).tobytes() + bytes(16)
    tables, axis = bytearray(), {}

    def table(cl, L):
        if (cl, L) not in axis:
            axis[(cl, L)] = len(tables)
            t = np.zeros((L + 3) // 4 * 4, dtype=np.uint32)
            t[:L] = LR.index(cl, L)
            tables.extend(t.tobytes())
        return axis[(cl, L)]

    run = run or max(1, 16384 // W)
    tasks = []
    for k, (si, box) in enumerate(jobs):
        h, w = srcs[si].shape
        x, y, bw, bh = box or (0, 0, w, h)
        sb = srcs[si].dtype.itemsize
        for y0 in range(0, H, run):
            t = LabelTask(src_off=soff[si] + (y * w + x) * sb, out_off=k * H * W * es, sx_off=table(bw, W), sy_off=table(bh, H),
                          src_pitch=w, out_w=W, out_h=H, row0=y0, rows=min(run, H - y0), src_bytes=sb,
                          dtype=list(LR.DTYPES).index(dtype))
            tasks.append(t)
    n = len(tasks)
    a = np.frombuffer(bytes(arena), dtype=np.uint8).copy()
    tb = _aligned(len(tables), 0)
    tb[:] = np.frombuffer(bytes(tables), dtype=np.uint8)
    slot = H * W * es
    out = _aligned(4096 + len(jobs) * slot + 4096, FILL)
    lt = (C.c_int32 * 256)(*[int(v) for v in lut]) if lut is not None else None
    assert launch("png_label_gather", a, out[4096:], (LabelTask * n)(*tasks), tb, lt, n, grid, emu=_emu) == 0
    assert (out[:4096] == FILL).all() and (out[4096 + len(jobs) * slot:] == FILL).all(), "the sentinel around the tensor was written"
    return out[4096: 4096 + len(jobs) * slot].view(LR.DTYPES[dtype]).reshape(len(jobs), H, W)


BOXES = [None, (0, 0, 10, 12), (35, 0, 10, 12), (0, 58, 10, 12), (35, 58, 10, 12), (20, 5, 1, 60), (44, 69, 1, 1)]
LUT = (np.random.default_rng(7).permutation(256).astype(np.int64) - 100)  # negative entries: sign extension
_SRC = {}


def _sources():
    if not _SRC:
        rng = np.random.default_rng(2)
        _SRC[1] = rng.integers(0, 256, size=(70, 45)).astype(np.uint8)
        _SRC[2] = rng.integers(0, 65536, size=(70, 45)).astype(np.uint16)
    return _SRC


@pytest.mark.parametrize("dtype", list(LR.DTYPES))
@pytest.mark.parametrize("size", [(1, 1), (5, 301), (130, 67)])
def test_gather_every_dtype_size_and_box(dtype, size):
    src = _sources()
    cases = [(1, None), (1, LUT if dtype in ("int32", "int64") else LUT + 100)]
    if dtype != "uint8":
        cases.append((2, None))
    for sb, lut in cases:
        jobs = [(0, b) for b in BOXES]
        got = run_gather([src[sb]], jobs, size, dtype, lut, run=None if size[0] < 100 else 7, grid=0 if size[0] < 100 else 5)
        for k, (_, box) in enumerate(jobs):
            exp = LR.gather(src[sb].astype(np.uint32), size, box, lut, dtype)
            assert got[k].dtype == exp.dtype and np.array_equal(got[k], exp), (dtype, size, sb, box, np.argwhere(got[k] != exp)[:4])


def test_gather_enlarging_40_times_and_the_identity():
    src = _sources()
    for dtype, sb in (("int64", 1), ("uint16", 2), ("uint8", 1), ("int32", 2)):
        got = run_gather([src[sb]], [(0, (7, 9, 3, 3)), (0, (42, 67, 3, 3))], (120, 120), dtype)
        for k, box in enumerate(((7, 9, 3, 3), (42, 67, 3, 3))):
            exp = LR.gather(src[sb].astype(np.uint32), (120, 120), box, None, dtype)
            assert np.array_equal(got[k], exp)
            assert np.array_equal(exp[::40, ::40], src[sb][box[1]: box[1] + 3, box[0]: box[0] + 3])
        same = run_gather([src[sb]], [(0, None)], (70, 45), dtype)
        assert np.array_equal(same[0], src[sb])


def test_gather_skips_tasks_that_break_a_bound():
    src = _sources()
    H, W = 6, 20
    base = dict(src_off=16, out_off=0, sx_off=0, sy_off=96, src_pitch=45, out_w=W, out_h=H, row0=0, rows=H, src_bytes=1, dtype=3)
    bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(src_bytes=3),
           dict(src_bytes=0), dict(dtype=4), dict(dtype=0, src_bytes=2), dict(sx_off=8), dict(sy_off=100), dict(src_bytes=2, src_off=17)]
    tasks = [LabelTask(**dict(base, **b)) for b in bad]
    a = np.zeros(16 + 70 * 45 * 2 + 16, dtype=np.uint8)
    a[16: 16 + 70 * 45] = src[1].reshape(-1)
    tb = _aligned(96 + 32, 0)
    tb.view(np.uint32)[:W] = LR.index(45, W)
    tb.view(np.uint32)[24: 24 + H] = LR.index(70, H)
    out = _aligned(4096 + H * W * 8 + 4096, FILL)
    n = len(tasks)
    assert _emu().emu_png_label_gather_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelTask * n)(*tasks), tb.ctypes.data, None, n, 0) == 0
    assert (out == FILL).all()
    lt = (C.c_int32 * 256)(*range(256))  # a LUT goes with one-byte labels only
    two = LabelTask(**dict(base, src_bytes=2))
    assert _emu().emu_png_label_gather_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelTask * 1)(two), tb.ctypes.data, lt, 1, 0) == 0
    assert (out == FILL).all()
    ok = LabelTask(**base)
    assert _emu().emu_png_label_gather_batch(a.ctypes.data, out.ctypes.data + 4096, (LabelTask * 1)(ok), tb.ctypes.data, lt, 1, 0) == 0
    got = out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W)
    assert np.array_equal(got, LR.gather(src[1].astype(np.uint32), (H, W)))


def test_kernels_under_address_sanitizer():
    """the same kernel sources under ASan + UBSan (tools/simt_emu/libdebig_emu_asan.so), in a child process"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(root)r)
import numpy as np
import test_emu_png_labels as E
E._check_index(E._index_images(13, sizes=[(1, 1), (7, 3), (13, 66)]))
src = E._sources()
for dtype, sb, size in (("uint8", 1, (5, 301)), ("uint16", 2, (9, 67)), ("int32", 1, (1, 1)), ("int64", 2, (33, 31))):
    lut = E.LUT + 100 if dtype == "uint8" else E.LUT if sb == 1 else None
    got = E.run_gather([src[sb]], [(0, b) for b in E.BOXES], size, dtype, lut, run=4)
    for k, box in enumerate(E.BOXES):
        assert np.array_equal(got[k], E.LR.gather(src[sb].astype(np.uint32), size, box, lut, dtype))
print("asan ok")
""" % {"root": root}
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", DEBIG_SPEC_EMU_ASAN="1")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "asan ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
