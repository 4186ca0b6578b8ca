"""The two label-distance kernels (csrc/png_label_distance_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy
restatement tests/png_label_distance_ref.py (a brute-force minimum over all sites per element; no passes, no envelopes):
  * run() lays the images out one behind the other -- labels, g planes and outputs each starting at a byte that is NOT a multiple of
    16 -- cuts each image into runs of rows and strips of columns, and launches the rows kernel and then the columns kernel through
    tests/stage_launch.py; check() compares every element of the g plane after the rows launch and every byte of the final output;
  * the g arena and the output lie between two sentinels of 4 KiB and are filled with a pattern before the launch, so a byte that no
    task owns must keep it; the label arena must come back unchanged, and the columns launch must leave the g arena unchanged;
  * every dtype x widths 1 .. 70 x six heights in both modes, lone sites, flat images, an absent value, alternating columns and
    short runs, runs that touch the top and the bottom, whole compares, caps, every seam, grids and orders, images without tasks,
    three long shapes, and the tasks that break a bound (emulator only)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_distance_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP = 0xEE, 4096
DTYPES = {"uint8": (0, np.uint8), "uint16": (1, np.uint16), "int32": (2, np.int32), "int64": (3, np.int64)}  # DEBIG_PNG_L_*
ROWS_ELEMS, COLS = 16384, 64  # include/debig_hip.h: DEBIG_PNG_LABEL_DISTANCE_ROWS_ELEMS, DEBIG_PNG_LABEL_DISTANCE_COLS
HEIGHTS = [1, 2, 3, 5, 17, 40]
FORMATS = {"squared": (0, np.int32), "root": (1, np.float32)}
ROWS, COLS_K = "png_label_distance_rows", "png_label_distance_cols"


class RowsTask(C.Structure):  # include/debig_hip.h: debig_png_label_distance_rows_task
    _fields_ = [("label_off", C.c_uint64), ("g_off", C.c_uint64), ("value", C.c_int64), ("w", C.c_uint32), ("h", C.c_uint32),
                ("row0", C.c_uint32), ("rows", C.c_uint32), ("dtype", C.c_uint32), ("sites", C.c_uint32)]


class ColsTask(C.Structure):  # include/debig_hip.h: debig_png_label_distance_cols_task
    _fields_ = [("g_off", C.c_uint64), ("out_off", C.c_uint64), ("w", C.c_uint32), ("h", C.c_uint32), ("x0", C.c_uint32),
                ("cols", C.c_uint32), ("cap", C.c_uint32), ("format", C.c_uint32)]


assert C.sizeof(RowsTask) == 48 and C.sizeof(ColsTask) == 40
_LIB = {}
_REF = {}  # the restatement of an image, computed once: (the image's values, its shape, to) -> (d2, none), never changed


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for name in ("emu_png_label_distance_rows_batch", "emu_png_label_distance_cols_batch"):
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(autouse=True)
def the_launchers_are_known(monkeypatch):
    """tests/stage_launch.py learns the two launchers for the length of one test (its table is another test's yardstick)"""
    monkeypatch.setitem(SL.KERNELS, ROWS, (SL.IN, SL.OUT, SL.TASKS))
    monkeypatch.setitem(SL.KERNELS, COLS_K, (SL.IN, SL.OUT, SL.TASKS))


def _aligned(n, fill):
    """n bytes of `fill` that start at a multiple of 64 (a view: the launch seam keeps the address's residue on the GPU)"""
    root = np.full(n + 64, fill, np.uint8)
    off = -root.ctypes.data % 64
    return root[off: off + n]


def ref(img, to):
    whole = R._whole(img).astype(np.int64)
    key = (whole.tobytes(), whole.shape, to)
    if key not in _REF:
        _REF[key] = R.d2(whole, to)
    return _REF[key]


def gref(img, to):
    whole = R._whole(img).astype(np.int64)
    key = (whole.tobytes(), whole.shape, to, "g")
    if key not in _REF:
        _REF[key] = R.row_g(whole, to)
    return _REF[key]


def host_run(W):
    """the rows of one task as debig_png_label_distance cuts them"""
    return 1 if W >= ROWS_ELEMS else ROWS_ELEMS // W


def run(images, to=None, cap=0, out="squared", rows=None, strip=COLS, grid=0, skip=(), spoil=None, keep_strip=None):
    """images: (H, W) arrays of one dtype; rows: the rows of a rows task (None: the host's cut); strip: the columns of a cols task;
    skip: images that get no task; spoil(rows tasks, cols tasks, owned): edits the lists; keep_strip(task) -> False drops a strip
    -> ([g plane (H, W) uint16 per image], [output (H, W) per image], rows tasks, cols tasks, [bool (H, W): owned by a cols task])"""
    code, npdt = next(v for v in DTYPES.values() if v[1] == images[0].dtype)
    es = np.dtype(npdt).itemsize
    fcode, odt = FORMATS[out]
    loff, goff, ooff, at, gt, ot = [], [], [], 0, GAP, GAP
    for img in images:  # every image, g plane and output image starts one element behind a multiple of 16 bytes
        at += -at % 16 + es
        loff.append(at)
        at += img.size * es
        gt += -gt % 16 + 2
        goff.append(gt)
        gt += img.size * 2
        ot += -ot % 16 + 4
        ooff.append(ot)
        ot += img.size * 4
    arena = _aligned(at, 0x5A)
    for img, o in zip(images, loff):
        assert o % 16 != 0 and arena[o:].ctypes.data % 16 != 0
        arena[o: o + img.size * es] = np.ascontiguousarray(img).reshape(-1).view(np.uint8)
    before = arena.copy()
    gbuf, buf = _aligned(gt + GAP, FILL), _aligned(ot + GAP, FILL)
    rtasks, ctasks, owned = [], [], [np.zeros(img.shape, bool) for img in images]
    for i, img in enumerate(images):
        if i in skip:
            continue
        H, W = img.shape
        per = rows or host_run(W)
        for y0 in range(0, H, per):
            rtasks.append(RowsTask(label_off=loff[i], g_off=goff[i], value=0 if to is None else to, w=W, h=H, row0=y0,
                                   rows=min(per, H - y0), dtype=code, sites=0 if to is None else 1))
        for x0 in range(0, W, strip):
            t = ColsTask(g_off=goff[i], out_off=ooff[i], w=W, h=H, x0=x0, cols=min(strip, W - x0), cap=cap, format=fcode)
            if keep_strip is None or keep_strip(t):
                ctasks.append(t)
                owned[i][:, x0: x0 + strip] = True
    if spoil:
        spoil(rtasks, ctasks, owned)
    assert SL.launch(ROWS, arena, gbuf, (RowsTask * max(len(rtasks), 1))(*rtasks), len(rtasks), grid, emu=_emu) == 0
    assert arena.tobytes() == before.tobytes(), "the label arena was written"
    assert (gbuf[:GAP] == FILL).all() and (gbuf[gt:] == FILL).all(), "a sentinel around the g planes was written"
    gs, at = [], GAP
    for img, o in zip(images, goff):
        assert (gbuf[at: o] == FILL).all(), "the bytes between two g planes were written"
        at = o + img.size * 2
        gs.append(gbuf[o: at].view(np.uint16).reshape(img.shape).copy())
    gbefore = gbuf.copy()
    assert SL.launch(COLS_K, gbuf, buf, (ColsTask * max(len(ctasks), 1))(*ctasks), len(ctasks), grid, emu=_emu) == 0
    assert gbuf.tobytes() == gbefore.tobytes(), "the columns launch wrote the g planes"
    assert (buf[:GAP] == FILL).all() and (buf[ot:] == FILL).all(), "a sentinel around the output was written"
    got, at = [], GAP
    for img, o in zip(images, ooff):
        assert (buf[at: o] == FILL).all(), "the bytes between two output images were written"
        at = o + img.size * 4
        got.append(buf[o: at].view(odt).reshape(img.shape).copy())
    return gs, got, rtasks, ctasks, owned


def check(images, to=None, cap=0, out="squared", skip=(), g_owned=None, **kw):
    gs, got, rtasks, ctasks, owned = run(images, to, cap, out, skip=skip, **kw)
    odt = FORMATS[out][1]
    for i, img in enumerate(images):
        pattern = np.frombuffer(bytes([FILL]) * (img.size * 4), odt).reshape(img.shape)
        gexp = gref(img, to) if i not in skip and g_owned is None else np.full(img.shape, FILL * 257, np.uint16)
        if g_owned is not None:
            gexp = np.where(g_owned[i], gref(img, to), gexp)
        assert gs[i].tobytes() == gexp.tobytes(), (i, img.shape, to, "g", np.argwhere(gs[i] != gexp)[:4])
        exp = np.where(owned[i], R.finish(*ref(img, to), cap, out), pattern)  # what no task owns keeps the fill pattern
        assert got[i].dtype == exp.dtype and got[i].tobytes() == exp.tobytes(), (
            i, img.shape, to, cap, out, kw.get("rows"), kw.get("strip"), kw.get("grid"),
            np.argwhere(got[i].view(np.uint32) != exp.view(np.uint32))[:4])
    return got, rtasks, ctasks


def _blocky(rng, H, W, dtype, block=5, ids=4):
    small = rng.integers(0, ids, (-(-H // block), -(-W // block)))
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:H, :W].astype(dtype)


# ---- dtypes and sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("to", [None, 1])
@pytest.mark.parametrize("name", list(DTYPES))
def test_every_dtype_width_and_height(name, to):
    """widths 1 .. 70 x six heights in two launches: blocky maps under the host's cut, noise in runs of 3 rows and strips of 16
    columns with three workgroups; no image's first byte is a multiple of 16.  The maps are the same for every dtype: the
    restatement is computed once"""
    rng = np.random.default_rng(7)
    npdt = DTYPES[name][1]
    blocky = [_blocky(rng, H, W, npdt) for i, W in enumerate(range(1, 71)) for H in (HEIGHTS[i % 6], HEIGHTS[(i + 3) % 6])]
    noise = [rng.integers(0, 3, (HEIGHTS[(i + 1) % 6], W)).astype(npdt) for i, W in enumerate(range(1, 71))]
    _, rt, ct = check(blocky, to)
    assert len(ct) > len(blocky) and len(rt) == len(blocky)
    check(noise, to, cap=3, out="root", rows=3, strip=16, grid=3)


# ---- sites -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", list(FORMATS))
def test_a_lone_site_in_every_corner_and_in_the_middle(out):
    H, W = 23, 37
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)):
        img = np.full((H, W), 4, np.int32)
        img[y, x] = 9
        yy, xx = np.mgrid[0:H, 0:W]
        want = (yy - y) ** 2 + (xx - x) ** 2
        for to in (None, 9):
            got, _, _ = check([img], to, 0, out, strip=16, rows=5)
            if to == 9:
                assert np.array_equal(got[0], want if out == "squared" else np.sqrt(want).astype(np.float32))
            else:  # the lone element's own nearest site is a neighbour
                assert got[0][y, x] == 1 and np.array_equal(np.delete(got[0].ravel(), y * W + x), np.delete(
                    (want if out == "squared" else np.sqrt(want).astype(np.float32)).ravel(), y * W + x))


def test_a_flat_image_and_an_absent_value_are_none():
    flat = [np.full((5, 70), 7, np.uint8), np.full((40, 3), 7, np.uint8), np.full((1, 1), 7, np.uint8)]
    for to in (None, 8, 256, -1):
        for cap, out, v in ((0, "squared", R.INT32_MAX), (0, "root", np.inf), (5, "squared", 25), (5, "root", 5.0), (32767, "squared", 32767 ** 2),
                            (32767, "root", 32767.0)):
            got, _, _ = check(flat, to, cap, out, strip=16)
            assert all((g == v).all() for g in got), (to, cap, out)
    # a value that int32 cannot hold, against elements that share its low word
    got, _, _ = check([np.full((4, 9), -1, np.int32)], 2 ** 32 - 1)
    assert (got[0] == R.INT32_MAX).all()
    assert (check([np.full((4, 9), -1, np.int32)], -1)[0][0] == 0).all()


# ---- the restarts of the envelope --------------------------------------------------------------------------------------------------------

def _columns(H, W, runs, dtype=np.uint8, seed=0):
    """columns whose values change after runs of the given lengths (cycled), with an offset per column"""
    img = np.zeros((H, W), dtype)
    for x in range(W):
        y, k, v = 0, x, x % 2
        while y < H:
            n = runs[k % len(runs)]
            img[y: y + n, x] = v
            y, k, v = y + n, k + 1, v + 1
    return img


@pytest.mark.parametrize("runs", [(1,), (2,), (3,), (1, 2, 3), (1, 7, 2), (5, 1, 1, 4)])
def test_columns_that_alternate_and_short_runs(runs):
    """every change of value down a column restarts the envelope, seeded and closed with the two virtual sites"""
    imgs = [_columns(H, 9, runs) for H in (1, 2, 3, 4, 7, 17)]
    check(imgs, None, strip=4)
    check(imgs, None, cap=1, out="root")
    check([im % 3 for im in imgs], 2, strip=4)


def test_a_run_that_touches_the_top_the_bottom_and_both():
    H, W = 17, 11
    top = np.zeros((H, W), np.uint16)
    top[6:] = 1                      # the upper run touches the top, the lower one the bottom
    top[6:, 4] = 0                   # ... and column 4 is one run that touches both
    top[3, 7] = 5                    # a site inside the upper run's rows
    mid = np.zeros((H, W), np.uint16)
    mid[5:12, 2:9] = 3               # a run that touches neither, rows whose g is none beside it
    both = np.zeros((H, W), np.uint16)
    both[:, 5] = 1                   # a column that differs from its neighbours over the whole height
    got, _, _ = check([top, mid, both], None, strip=5, rows=4)
    assert got[0][0, 0] == 36 and got[0][16, 0] == 16 and got[2][9, 0] == 25
    check([top, mid, both], 1)
    check([top, mid, both], 3, cap=5, out="root")


# ---- values ------------------------------------------------------------------------------------------------------------------------------

def test_elements_are_compared_whole():
    a = np.full((9, 9), 3, np.int64)
    a[4, 4] = 2 ** 32 + 3  # the low word is equal
    b = np.full((9, 9), -1, np.int64)
    b[4, 4] = 255
    c = np.full((9, 9), 2 ** 40, np.int64)
    c[4, 4] = 2 ** 40 + 2 ** 32
    got, _, _ = check([a, b, c], None)
    yy, xx = np.mgrid[0:9, 0:9]
    want = (yy - 4) ** 2 + (xx - 4) ** 2
    want[4, 4] = 1
    assert all(np.array_equal(g, want) for g in got)
    want[4, 4] = 0
    assert np.array_equal(check([a], 2 ** 32 + 3)[0][0], want) and (check([a], 3)[0][0] == (want == 0)).all()
    assert np.array_equal(check([b], 255)[0][0], want) and np.array_equal(check([c], 2 ** 40 + 2 ** 32)[0][0], want)
    d = np.full((9, 9), -1, np.int32)
    d[4, 4] = 255
    assert np.array_equal(check([d], 255)[0][0], want) and (check([d], -1)[0][0] == (want == 0)).all()
    e = np.full((9, 9), 0xFFFF, np.uint16)
    e[4, 4] = 0x00FF
    assert np.array_equal(check([e], 255)[0][0], want) and (check([e], -1)[0][0] == R.INT32_MAX).all()
    f = np.full((9, 9), 255, np.uint8)
    assert (check([f], -1)[0][0] == R.INT32_MAX).all() and (check([f], 255)[0][0] == 0).all()


@pytest.mark.parametrize("cap", [1, 5, 32767])
def test_caps(cap):
    rng = np.random.default_rng(3)
    imgs = [_blocky(rng, 40, 70, np.uint8, block=13), np.full((6, 6), 1, np.uint8)]
    imgs[0][0, 0] = 200
    for out in FORMATS:
        for to in (None, 200):
            got, _, _ = check(imgs, to, cap, out)
            assert got[0].max() == (min(cap * cap, ref(imgs[0], to)[0].max()) if out == "squared" else min(
                cap, np.float32(np.sqrt(float(ref(imgs[0], to)[0].max())))))
            assert (got[1] == (cap * cap if out == "squared" else cap)).all()


# ---- the cut, the grid and the order -----------------------------------------------------------------------------------------------------

def _seams(npdt, strip, rows, H=40, W=70):
    img = np.full((H, W), 3, npdt)
    for x in range(strip, W, strip):  # both sides of every vertical seam
        img[7, x - 1], img[21, x] = 20, 21
    for y in range(rows, H, rows):  # ... and of every horizontal one
        img[y - 1, 5], img[y, 50] = 22, 23
    return img


@pytest.mark.parametrize("name", ["uint8", "int64"])
def test_strips_and_row_runs_cut_at_every_seam(name):
    """70 x 40: every strip width 1 .. 70 and every run of rows 1 .. 40 gives the bytes of the host's cut"""
    rng = np.random.default_rng(12)
    npdt = DTYPES[name][1]
    noisy = _blocky(rng, 40, 70, npdt, block=9)
    first = {}
    for k in range(1, 71):
        strip, rows = min(k, COLS), (k - 1) % 40 + 1
        for to in (None, 21):
            imgs = [_seams(npdt, strip, rows), noisy]
            got, rt, ct = check(imgs, to, rows=rows, strip=strip, grid=k % 4)
            assert len(rt) == 2 * -(-40 // rows) and len(ct) == 2 * -(-70 // strip)
            first.setdefault(to, got[1])
            assert got[1].tobytes() == first[to].tobytes()


def _mixed(name):
    rng = np.random.default_rng(11)
    npdt = DTYPES[name][1]
    return [_blocky(rng, 24, 33, npdt), rng.integers(0, 4, (24, 33)).astype(npdt), _blocky(rng, 5, 70, npdt, block=3),
            np.full((24, 9), 2, npdt), _blocky(rng, 40, 70, npdt, block=7)]


def _order(kind):
    def spoil(rtasks, ctasks, owned):
        if kind == "reversed":
            rtasks.reverse()
            ctasks.reverse()
        else:
            rng = np.random.default_rng(5)
            rtasks[:] = [rtasks[i] for i in rng.permutation(len(rtasks))]
            ctasks[:] = [ctasks[i] for i in rng.permutation(len(ctasks))]
    return spoil


@pytest.mark.parametrize("name", ["uint16", "int32"])
def test_fewer_workgroups_than_tasks_in_both_orders(name):
    images = _mixed(name)
    first = None
    for grid in (0, 1, 2, 5):
        for spoil in (None, _order("reversed"), _order("shuffled")):
            got, rt, ct = check(images, None, 16, "root", rows=7, strip=8, grid=grid, spoil=spoil)
            first = first or got
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
            assert len(rt) > 5 and len(ct) > 5
    check(images, 2, rows=7, strip=8, grid=2, spoil=_order("reversed"))


def test_a_launch_over_half_the_strips_writes_only_those():
    images = _mixed("uint8")
    got, _, ct = check(images, None, strip=8, keep_strip=lambda t: (t.x0 // 8) % 2 == 0, grid=2)
    assert len(ct) > 10 and any((g.view(np.uint8) == FILL).all(axis=0).any() for g in got)


def test_images_without_tasks_keep_the_pattern():
    images = _mixed("uint16")
    got, rt, ct = check(images, None, skip=(1, 4), strip=16, rows=5, grid=2)
    assert (got[1].view(np.uint8) == FILL).all() and (got[4].view(np.uint8) == FILL).all() and rt and ct
    got, rt, ct = check(images, 2, out="root", skip=range(5))
    assert rt == [] and ct == [] and all((g.view(np.uint8) == FILL).all() for g in got)


# ---- the long shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 16384), (16384, 3), (16384, 1)])
def test_long_shapes(shape):
    """3 x 16384: the row scan's carries over 256 segments and the largest row distance; under ROOT the values k^2 + 1 and k^2 + 4
    above 2^24, where sqrtf((float)d2) is not the nearest float32.  16384 x 3 and 16384 x 1: the longest envelope, the stack at its
    full depth (every row of column 1 and 2 is a site of its own under TO_VALUE)"""
    H, W = shape
    img = np.zeros(shape, np.uint8)
    img[H - 1, W - 1] = 1
    for to in (None, 1):
        got, _, _ = check([img], to, 0, "root")
        check([img], to, 0, "squared")
    if shape == (3, 16384):
        d2 = ref(img, 1)[0]
        naive = np.sqrt(d2.astype(np.float32))
        assert (d2 > 2 ** 24).sum() > 30000 and (naive != got[0]).any()  # the two square-root rules part here


@pytest.mark.parametrize("H", [2048, 16384])
def test_the_stack_at_full_depth(H):
    """a first column of ones: every row of a column has the same row distance, so every row's parabola stays on the envelope
    and the stack grows to one entry per row.  The result is known without the restatement: D2 = x^2 towards the ones, and under
    DIFFERS 1 for the ones' own column"""
    img = np.zeros((H, 3), np.uint8)
    img[:, 0] = 1
    gs, got, _, _, _ = run([img], 1)
    assert np.array_equal(gs[0], np.broadcast_to(np.arange(3, dtype=np.uint16), (H, 3)))
    assert got[0].dtype == np.int32 and np.array_equal(got[0], np.broadcast_to(np.array([0, 1, 4], np.int32), (H, 3)))
    gs, got, _, _, _ = run([img], None, out="root")
    assert np.array_equal(gs[0], np.broadcast_to(np.array([1, 1, 2], np.uint16), (H, 3)))
    assert got[0].dtype == np.float32 and np.array_equal(got[0], np.broadcast_to(np.array([1, 1, 2], np.float32), (H, 3)))
    if H == 2048:  # ... and growing and shrinking row distances against the restatement
        stair = np.zeros((H, 3), np.uint8)
        stair[:, 0] = np.arange(H) % 2 + 1
        stair[H // 3, 2] = 1
        check([stair], None)
        check([stair[::-1].copy()], 2)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------

def test_tasks_that_break_a_bound_are_skipped():
    """every bound of include/debig_hip.h, one task each, between good tasks: what the bad task owns keeps the pattern, the good
    tasks' elements are right, the sentinels stay"""
    rng = np.random.default_rng(5)
    images = [_blocky(rng, 24, 33, np.int32), _blocky(rng, 24, 33, np.int32)]

    def broken_rows(field, value):
        def spoil(rtasks, ctasks, owned):
            bad = RowsTask.from_buffer_copy(bytes(rtasks[0]))
            setattr(bad, field, value(bad))
            rtasks[:] = [bad, rtasks[1], bad]
            ctasks[:] = [t for t in ctasks if t.g_off == rtasks[1].g_off]
            owned[0][:] = False
        return spoil

    g_owned = [np.zeros((24, 33), bool), np.ones((24, 33), bool)]
    rows_cases = [("dtype", lambda t: 4), ("dtype", lambda t: 2 ** 31), ("sites", lambda t: 2), ("sites", lambda t: 2 ** 32 - 1),
                  ("w", lambda t: 0), ("w", lambda t: 16385), ("h", lambda t: 0), ("h", lambda t: 16385), ("rows", lambda t: 0),
                  ("rows", lambda t: 25), ("row0", lambda t: 24), ("row0", lambda t: 1), ("row0", lambda t: 2 ** 32 - 1),
                  ("rows", lambda t: 2 ** 32 - 1), ("label_off", lambda t: t.label_off + 1), ("label_off", lambda t: t.label_off + 2),
                  ("g_off", lambda t: t.g_off + 1)]
    for field, value in rows_cases:
        for grid in (0, 1):
            _, rt, _ = check(images, None, rows=24, grid=grid, spoil=broken_rows(field, value), g_owned=g_owned)
            assert len(rt) == 3
    # a run of more than 16384 elements in more than one row
    wide = [np.zeros((4, 5000), np.uint8), np.zeros((4, 5000), np.uint8)]
    wide[1][2, 77] = 1
    check(wide, None, rows=4, spoil=broken_rows("w", lambda t: t.w), g_owned=[np.zeros((4, 5000), bool)] * 2, keep_strip=lambda t: False)
    check(wide, None, rows=3, keep_strip=lambda t: t.x0 == 64)

    def broken_cols(field, value):
        def spoil(rtasks, ctasks, owned):
            bad = ColsTask.from_buffer_copy(bytes(ctasks[0]))
            setattr(bad, field, value(bad))
            ctasks[:] = [bad, ctasks[1], bad]
            owned[0][:] = False
        return spoil

    cols_cases = [("format", lambda t: 2), ("format", lambda t: 2 ** 31), ("cap", lambda t: 32768), ("cap", lambda t: 2 ** 32 - 1),
                  ("w", lambda t: 0), ("w", lambda t: 16385), ("h", lambda t: 0), ("h", lambda t: 16385), ("cols", lambda t: 0),
                  ("cols", lambda t: 65), ("cols", lambda t: 34), ("x0", lambda t: 33), ("x0", lambda t: 1), ("x0", lambda t: 2 ** 32 - 1),
                  ("cols", lambda t: 2 ** 32 - 1), ("g_off", lambda t: t.g_off + 1), ("out_off", lambda t: t.out_off + 1),
                  ("out_off", lambda t: t.out_off + 2)]
    for field, value in cols_cases:
        for grid in (0, 1):
            _, _, ct = check(images, None, strip=COLS, grid=grid, spoil=broken_cols(field, value))
            assert len(ct) == 3
