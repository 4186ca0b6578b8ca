"""The label-boundary kernel (csrc/png_label_boundary_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy
restatement tests/png_label_boundary_ref.py (shifted compares over the footprint; no tiles, no passes):
  * run() lays the images out one behind the other, every image (input and output) starting at a byte that is NOT a multiple of
    16, cuts each image into tiles, and launches once through tests/stage_launch.py; check() compares every output byte;
  * the output lies between two sentinels of 4 KiB and is filled with a pattern before the launch, so a byte that no task owns
    must keep it; the label arena must come back unchanged;
  * every dtype x widths 1 .. 70 x a spread of heights, a lone element under every radius x shape (the marked set is exactly the
    footprint), images smaller than the radius, corners and tile seams, tiles of 5 x 3 under r = 16, the ends of every dtype, both
    modes, every cut x grid x order, half the tiles, images without tasks, and the tasks that break a bound (emulator only)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_boundary_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP = 0xEE, 4096
DTYPES = {"uint8": (0, np.uint8), "uint16": (1, np.uint16), "int32": (2, np.int32), "int64": (3, np.int64)}  # DEBIG_PNG_L_*
MAX_TILE, LDS_BYTES = 128, 40960  # include/debig_hip.h: DEBIG_PNG_LABEL_BOUNDARY_MAX_TILE, _LDS_BYTES
HEIGHTS = [1, 2, 3, 5, 17, 40]


class BoundaryTask(C.Structure):  # include/debig_hip.h: debig_png_label_boundary_task
    _fields_ = [("label_off", C.c_uint64), ("out_off", C.c_uint64), ("value", C.c_int64), ("w", C.c_uint32), ("h", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("dtype", C.c_uint32),
                ("mode", C.c_uint32), ("radius", C.c_uint32), ("reach", C.c_uint8 * 17), ("reserved", C.c_uint8 * 3)]


assert C.sizeof(BoundaryTask) == 80
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_label_boundary_batch.restype = C.c_int
        L.emu_png_label_boundary_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(autouse=True)
def the_launcher_is_known(monkeypatch):
    """tests/stage_launch.py learns the launcher for the length of one test (its table is another test's yardstick)"""
    monkeypatch.setitem(SL.KERNELS, "png_label_boundary", (SL.IN, SL.OUT, SL.TASKS))


def _aligned(n, fill):
    """n bytes of `fill` that start at a multiple of 64 (a view: the launch seam keeps the address's residue on the GPU)"""
    root = np.full(n + 64, fill, np.uint8)
    off = -root.ctypes.data % 64
    return root[off: off + n]


def lds_bytes(tw, th, es, r):
    """include/debig_hip.h: DEBIG_PNG_LABEL_BOUNDARY_TILE_BYTES"""
    pitch = ((tw + 2 * r) * es + 30) & ~15
    return (th + 2 * r) * (pitch + ((pitch // es + 15) & ~15))


def host_tile(es, r):
    """the tile debig_png_label_boundary cuts"""
    tw, th = 128, 64
    while lds_bytes(tw, th, es, r) > LDS_BYTES:
        if tw > th:
            tw //= 2
        else:
            th //= 2
    return tw, th


def run(images, radius, shape="square", mode="ring", value=255, tile=None, grid=0, spoil=None, skip=(), table=None, keep=None):
    """images: (H, W) arrays of one dtype; tile: (tile_w, tile_h) (None: the host's cut); skip: images that get no task;
    table: a reach table instead of the shape's; keep(task) -> False drops a tile's task
    -> ([output (H, W) per image], the task list, [bool (H, W) per image: the elements some task owns])"""
    code, npdt = next(v for v in DTYPES.values() if v[1] == images[0].dtype)
    es = np.dtype(npdt).itemsize
    odt = np.uint8 if mode == "edge" else npdt
    os_ = np.dtype(odt).itemsize
    table = R.reach(radius, shape) if table is None else list(table)
    loff, ooff, at, ot = [], [], 0, GAP
    for img in images:  # every image, and every output image, starts one element behind a multiple of 16 bytes
        at += -at % 16 + es
        loff.append(at)
        at += img.size * es
        ot += -ot % 16 + os_
        ooff.append(ot)
        ot += img.size * os_
    arena = _aligned(at, 0x5A)
    for img, o in zip(images, loff):
        assert o % 16 != 0 and arena[o:].ctypes.data % 16 != 0
        arena[o: o + img.size * es] = np.ascontiguousarray(img).reshape(-1).view(np.uint8)
    before = arena.copy()
    buf = _aligned(ot + GAP, FILL)
    tw, th = tile or host_tile(es, radius)
    tasks, owned = [], [np.zeros(img.shape, bool) for img in images]
    for i, img in enumerate(images):
        if i in skip:
            continue
        H, W = img.shape
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                t = BoundaryTask(label_off=loff[i], out_off=ooff[i], value=value, w=W, h=H, x0=x0, y0=y0, tile_w=min(tw, W - x0),
                                 tile_h=min(th, H - y0), dtype=code, mode=R.MODES[mode], radius=radius)
                for d, v in enumerate(table):
                    t.reach[d] = v
                if keep is None or keep(t):
                    tasks.append(t)
                    owned[i][y0: y0 + th, x0: x0 + tw] = True
    if spoil:
        spoil(tasks, owned)
    n = len(tasks)
    arr = (BoundaryTask * max(n, 1))(*tasks)
    assert SL.launch("png_label_boundary", arena, buf, arr, n, grid, emu=_emu) == 0
    assert arena.tobytes() == before.tobytes(), "the label arena was written"
    assert (buf[:GAP] == FILL).all() and (buf[ot:] == FILL).all(), "a sentinel around the output was written"
    got, at = [], GAP
    for img, o in zip(images, ooff):
        assert (buf[at: o] == FILL).all(), "the bytes between two output images were written"
        at = o + img.size * os_
        got.append(buf[o: at].view(odt).reshape(img.shape).copy())
    return got, tasks, owned


def want(img, radius, shape, mode, value, table=None):
    return R.apply_image(img, R.reach(radius, shape) if table is None else list(table), mode, value)


def check(images, radius, shape="square", mode="ring", value=255, skip=(), table=None, **kw):
    got, tasks, owned = run(images, radius, shape, mode, value, skip=skip, table=table, **kw)
    odt = np.uint8 if mode == "edge" else images[0].dtype
    for i, img in enumerate(images):
        exp = want(img, radius, shape, mode, value, table)
        pattern = np.frombuffer(bytes([FILL]) * (img.size * np.dtype(odt).itemsize), odt).reshape(img.shape)
        exp = np.where(owned[i], exp, pattern)  # what no task owns keeps the fill pattern
        assert got[i].dtype == exp.dtype and got[i].tobytes() == exp.tobytes(), (
            i, img.shape, radius, shape, mode, kw.get("tile"), kw.get("grid"), np.argwhere(got[i] != exp)[:4])
    return got, tasks


def _blocky(rng, H, W, dtype, block=5, ids=6):
    small = rng.integers(0, ids, (-(-H // block), -(-W // block)))
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:H, :W].astype(dtype)


# ---- dtypes and sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ring", "edge"])
@pytest.mark.parametrize("name", list(DTYPES))
def test_every_dtype_width_and_height(name, mode):
    """widths 1 .. 70 x six heights in two launches: blocky maps under the square of radius 2 in tiles of 32 x 32, noise under the
    disk of radius 3 in tiles of 16 x 8; no image's first byte is a multiple of 16"""
    rng = np.random.default_rng(DTYPES[name][0])
    npdt = DTYPES[name][1]
    blocky = [_blocky(rng, H, W, npdt) for i, W in enumerate(range(1, 71)) for H in (HEIGHTS[i % 6], HEIGHTS[(i + 3) % 6])]
    noise = [rng.integers(0, 3, (HEIGHTS[(i + 1) % 6], W)).astype(npdt) for i, W in enumerate(range(1, 71))]
    _, tasks = check(blocky, 2, "square", mode, 200, tile=(32, 32))
    assert len(tasks) > len(blocky)
    check(noise, 3, "disk", mode, 7, tile=(16, 8), grid=3)


# ---- the footprint -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_a_lone_element_marks_exactly_the_footprint(shape):
    """one differing element in the middle of a flat 35 x 35 map, every radius: the marked set is the footprint around it (the
    rule is symmetric), which pins every reach entry and both off-by-ones"""
    for radius in range(1, R.MAX_RADIUS + 1):
        img = np.full((35, 35), 4, np.int32)
        img[17, 17] = 9
        got, _ = check([img], radius, shape, "edge", tile=(32, 32) if radius % 2 else (7, 9))
        mark = np.zeros((35, 35), bool)
        mark[17 - radius: 18 + radius, 17 - radius: 18 + radius] = R.footprint(radius, shape)
        assert np.array_equal(got[0].astype(bool), mark), (radius, shape)
        ring, _ = check([img.astype(np.uint8)], radius, shape, "ring", 255)
        assert np.array_equal(ring[0] == 255, mark)


def test_images_smaller_than_the_radius():
    for name in ("uint8", "int64"):
        npdt = DTYPES[name][1]
        one = np.array([[5]], npdt)
        row = np.array([[1, 1, 1, 2, 2, 2, 2]], npdt)
        col = np.array([[3], [3], [3], [3], [4], [3], [3], [3], [3]], npdt)
        for radius in (1, 2, 5, 16):
            for shape in R.SHAPES:
                for mode in R.MODES:
                    got, _ = check([one, row, col], radius, shape, mode, 77)
        assert got[0].tolist() == [[0]] and got[1].all() and got[2].all()  # r = 16: everything sees the other id; 1 x 1 nothing


# ---- corners, seams, thin tiles ----------------------------------------------------------------------------------------------------------

def _corners_and_seams(npdt, tw, th, H=40, W=70):
    img = np.full((H, W), 3, npdt)
    img[0, 0], img[0, -1], img[-1, 0], img[-1, -1] = 10, 11, 12, 13
    for x in range(tw, W, tw):  # both sides of every vertical seam
        img[7, x - 1], img[21, x] = 20, 21
    for y in range(th, H, th):  # ... and of every horizontal one
        img[y - 1, 5], img[y, 50] = 22, 23
    return img


@pytest.mark.parametrize("name", list(DTYPES))
def test_corners_and_both_sides_of_every_seam(name):
    for tw, th in ((32, 32), (16, 8), (64, 32)):
        img = _corners_and_seams(DTYPES[name][1], tw, th)
        for radius, shape in ((1, "square"), (1, "diamond"), (3, "disk"), (8, "square")):
            check([img], radius, shape, "ring", 255, tile=(tw, th))
            check([img], radius, shape, "edge", tile=(tw, th), grid=2)


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_tiles_of_5_by_3_under_radius_16(shape):
    """the halo of a tile spans several tiles on every side"""
    rng = np.random.default_rng(8)
    imgs = [_blocky(rng, 24, 33, np.uint16, block=11), _blocky(rng, 17, 40, np.uint16, block=9)]
    _, tasks = check(imgs, 16, shape, "ring", 65535, tile=(5, 3))
    assert len(tasks) == 7 * 8 + 8 * 6
    check([im.astype(np.int64) for im in imgs], 16, shape, "edge", tile=(5, 3), grid=3)


# ---- values ------------------------------------------------------------------------------------------------------------------------------

def test_elements_are_compared_whole():
    a = np.full((9, 9), 3, np.int64)
    a[4, 4] = 2 ** 32 + 3  # the low word is equal
    b = np.full((9, 9), -1, np.int64)
    b[4, 4] = np.iinfo(np.int64).max  # ... and here the high word nearly
    c = np.full((9, 9), 2 ** 40, np.int64)
    c[4, 4] = 2 ** 40 + 2 ** 32
    got, _ = check([a, b, c], 1, "diamond", "edge")
    for g in got:
        assert g.sum() == 5
    d = np.full((9, 9), np.iinfo(np.int32).min, np.int32)
    d[4, 4] = 0
    e = np.full((9, 9), 0xFFFF, np.uint16)
    e[4, 4] = 0x00FF
    assert check([d], 1, "square", "edge")[0][0].sum() == 9 and check([e], 1, "square", "edge")[0][0].sum() == 9
    flat = np.full((9, 9), -1, np.int64)
    assert not check([flat], 16, "square", "edge")[0][0].any()


@pytest.mark.parametrize("name", list(DTYPES))
def test_value_at_both_ends_of_the_dtype_and_equal_to_an_id(name):
    npdt = DTYPES[name][1]
    rng = np.random.default_rng(2)
    img = _blocky(rng, 17, 33, npdt)
    for value in (np.iinfo(npdt).min, np.iinfo(npdt).max, int(img[0, 0]), 0):
        got, _ = check([img], 2, "disk", "ring", int(value))
        b = R.boundary(img, R.reach(2, "disk"))
        assert b.any() and not b.all() and (got[0][b] == value).all() and (got[0][~b] == img[~b]).all()


# ---- the tile cut, the grid and the order ------------------------------------------------------------------------------------------------

def _shuffled(seed):
    def spoil(tasks, owned):
        rng = np.random.default_rng(seed)
        tasks[:] = [tasks[i] for i in rng.permutation(len(tasks))]
    return spoil


def _mixed(name):
    rng = np.random.default_rng(11)
    npdt = DTYPES[name][1]
    return [_blocky(rng, 24, 33, npdt), rng.integers(0, 4, (24, 33)).astype(npdt), _blocky(rng, 5, 70, npdt, block=3),
            np.full((24, 9), 2, npdt), _blocky(rng, 40, 70, npdt, block=7)]


@pytest.mark.parametrize("name", ["uint8", "int64"])
def test_every_cut_grid_and_order_gives_the_same_bytes(name):
    images = _mixed(name)
    first = None
    for tile in ((5, 3), (16, 8), (32, 32), (70, 40), None):
        for grid in (0, 1, 2, 3):
            for spoil in (None, _shuffled(grid + 1)):
                if tile == (5, 3) and (grid == 0 or spoil):
                    continue  # (the many small tiles once per grid)
                got, tasks = check(images, 3, "disk", "ring", 255, tile=tile, grid=grid, spoil=spoil)
                first = first or got
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
                assert grid == 0 or len(tasks) > grid


def test_the_host_cut_fits_and_32_by_32_always_does():
    for es in (1, 2, 4, 8):
        for r in range(1, 17):
            assert lds_bytes(32, 32, es, r) <= LDS_BYTES
            tw, th = host_tile(es, r)
            assert lds_bytes(tw, th, es, r) <= LDS_BYTES and 32 <= tw <= MAX_TILE and 32 <= th <= MAX_TILE
    assert host_tile(1, 1) == (128, 64) and host_tile(8, 16) == (32, 32)


@pytest.mark.parametrize("name", ["uint8", "int64"])
def test_the_largest_tiles_of_the_host_cut(name):
    """200 x 150 under the host's own tiles (128 x 64 for uint8 at r = 1, 32 x 32 for int64 at r = 16): whole tiles and cut ones"""
    rng = np.random.default_rng(4)
    img = _blocky(rng, 150, 200, DTYPES[name][1], block=23)
    for radius in (1, 16):
        check([img], radius, "square", "ring", 255)
    check([img], 16, "disk", "edge", grid=2)


# ---- partial launches --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["ring", "edge"])
def test_a_launch_over_half_the_tiles_writes_only_those(mode):
    images = _mixed("int32")
    got, tasks = check(images, 2, "square", mode, 255, tile=(16, 8), keep=lambda t: (t.x0 // 16 + t.y0 // 8) % 2 == 0, grid=2)
    assert len(tasks) > 10
    full = run(images, 2, "square", mode, 255, tile=(16, 8))[0]
    assert any(a.tobytes() != b.tobytes() for a, b in zip(got, full))


def test_images_without_tasks_keep_the_pattern():
    images = _mixed("uint16")
    got, tasks = check(images, 1, "diamond", "ring", 255, skip=(1, 4), tile=(32, 32), grid=2)
    assert (got[1].view(np.uint8) == FILL).all() and (got[4].view(np.uint8) == FILL).all() and tasks
    got, tasks = check(images, 1, "diamond", "edge", skip=range(5))
    assert tasks == [] and all((g == FILL).all() for g in got)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------

def test_tasks_that_break_a_bound_are_skipped():
    """every bound of include/debig_hip.h, one task each, between two good tasks: the bad task's tile keeps the pattern, the good
    tasks' tiles are right, the sentinels stay"""
    rng = np.random.default_rng(5)
    images = [_blocky(rng, 24, 33, np.int32), _blocky(rng, 24, 33, np.int32)]

    def broken(field, value):
        def spoil(tasks, owned):
            bad = BoundaryTask.from_buffer_copy(bytes(tasks[0]))
            if field == "reach":
                bad.reach[value(bad)] = bad.radius + 1
            else:
                setattr(bad, field, value(bad))
            tasks[:] = [bad, tasks[1], bad]
            owned[0][:] = False
        return spoil

    cases = [("dtype", lambda t: 4), ("dtype", lambda t: 255), ("mode", lambda t: 2), ("mode", lambda t: 2 ** 31), ("radius", lambda t: 0),
             ("radius", lambda t: 17), ("radius", lambda t: 2 ** 32 - 1), ("reach", lambda t: 0), ("reach", lambda t: 2),
             ("w", lambda t: 0), ("w", lambda t: 16385), ("h", lambda t: 0), ("h", lambda t: 16385), ("tile_w", lambda t: 0),
             ("tile_h", lambda t: 0), ("tile_w", lambda t: 34), ("tile_h", lambda t: 25), ("x0", lambda t: 1), ("x0", lambda t: 33),
             ("y0", lambda t: 24), ("y0", lambda t: 2 ** 32 - 1), ("x0", lambda t: 2 ** 32 - 1), ("tile_w", lambda t: 2 ** 32 - 1),
             ("tile_w", lambda t: MAX_TILE + 1), ("tile_h", lambda t: MAX_TILE + 1), ("value", lambda t: 2 ** 31), ("value", lambda t: -2 ** 31 - 1),
             ("label_off", lambda t: t.label_off + 1), ("label_off", lambda t: t.label_off + 2), ("out_off", lambda t: t.out_off + 1),
             ("out_off", lambda t: t.out_off + 2)]
    for field, value in cases:
        for grid in (0, 1):
            _, tasks = check(images, 2, "square", "ring", 9, tile=(33, 24), grid=grid, spoil=broken(field, value))
            assert len(tasks) == 3
    # the value ranges of the narrow dtypes; under EDGE the value is not looked at
    for name, bad_values in (("uint8", (-1, 256)), ("uint16", (-1, 65536))):
        imgs = [im.astype(DTYPES[name][1]) for im in images]
        for v in bad_values:
            check(imgs, 2, "square", "ring", 9, tile=(33, 24), spoil=broken("value", lambda t, v=v: v))
    got = run(images, 2, "square", "edge", 9, tile=(33, 24), spoil=lambda tasks, owned: setattr(tasks[0], "value", 2 ** 40))[0]
    assert got[0].tobytes() == want(images[0], 2, "square", "edge", 9).tobytes()
    # a tile whose planes exceed the LDS cap: 128 x 128 of int64 under r = 16, inside a large enough image
    big = np.zeros((160, 160), np.int64)
    big[80, 80] = 1
    assert lds_bytes(128, 128, 8, 16) > LDS_BYTES

    def too_large(tasks, owned):
        t = BoundaryTask.from_buffer_copy(bytes(tasks[0]))
        t.tile_w = t.tile_h = 128
        tasks[:] = [t]
        owned[0][:] = False
    check([big], 16, "square", "ring", 9, tile=(32, 32), spoil=too_large)
