"""The label-statistics kernel (csrc/png_label_stats_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the numpy
restatement tests/png_label_stats_ref.py (RAW records, include/debig_hip.h: debig_png_label_stat):
  * run() lays the images out as a dense tensor would (an image's rows one behind the other) but starts every image at an element
    offset that leaves its first byte unaligned to 16, cuts the row runs as the host does (or into `run` rows), and launches once
    through tests/stage_launch.py; check() compares every record;
  * the record buffer lies between two sentinels of 4 KiB, which must stay; the label arena must come back unchanged;
  * every dtype, sizes from 1 x 1, the ends of the id range, patterns that pile onto one entry or change id at every element,
    every task cut, grids 0 .. 3 and a shuffled task order, two images of different n_ids through one workgroup, images without
    tasks, records accumulated over two launches, and the tasks that break a bound (emulator only)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_stats_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP = 0xEE, 4096
DTYPES = {"uint8": (0, np.uint8), "uint16": (1, np.uint16), "int32": (2, np.int32), "int64": (3, np.int64)}  # DEBIG_PNG_L_*
HOST_RUN = 16384  # include/debig_hip.h: DEBIG_PNG_LABEL_STATS_RUN
WIDTHS, HEIGHTS = [1, 7, 9, 33, 70], [1, 5, 24]


class StatsTask(C.Structure):  # include/debig_hip.h: debig_png_label_stats_task
    _fields_ = [("label_off", C.c_uint64), ("stat_off", C.c_uint64), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("row0", C.c_uint32), ("rows", C.c_uint32), ("n_ids", C.c_uint32), ("dtype", C.c_uint32)]


assert C.sizeof(StatsTask) == 40
_LIB = {}


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        L.emu_png_label_stats_batch.restype = C.c_int
        L.emu_png_label_stats_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(autouse=True)
def the_launcher_is_known(monkeypatch):
    """tests/stage_launch.py learns the launcher for the length of one test (its table is another test's yardstick)"""
    monkeypatch.setitem(SL.KERNELS, "png_label_stats", (SL.IN, SL.OUT, SL.TASKS))


def _aligned(n, fill):
    """n bytes of `fill` that start at a multiple of 64 (a view: the launch seam keeps the address's residue on the GPU)"""
    root = np.full(n + 64, fill, np.uint8)
    off = -root.ctypes.data % 64
    return root[off: off + n]


def run(images, n_ids, run=None, grid=0, spoil=None, skip=(), into=None, rows_of=None):
    """images: (H, W) arrays of one dtype; n_ids: one number or one per image; run: rows of a task (None: the host's cut);
    skip: images that get no task; into: (records buffer, offsets) of an earlier call, to accumulate into; rows_of(i, H): the
    (row0, rows) range of image i that is cut into tasks (default: all rows)
    -> ([raw records (n_ids + 1, 5) uint32 per image], the task list, (records buffer, offsets))"""
    code, npdt = next(v for v in DTYPES.values() if v[1] == images[0].dtype)
    es = np.dtype(npdt).itemsize
    ids = [n_ids] * len(images) if isinstance(n_ids, int) else list(n_ids)
    loff, at = [], 0
    for img in images:  # every image starts one element behind a multiple of 16 bytes
        at += -at % 16 + es
        loff.append(at)
        at += img.size * es
    arena = _aligned(at, 0x5A)
    for img, o in zip(images, loff):
        assert o % 16 != 0 and arena[o:].ctypes.data % 16 != 0
        arena[o: o + img.size * es] = np.ascontiguousarray(img).reshape(-1).view(np.uint8)
    before = arena.copy()
    if into is None:
        soff, at = [], GAP
        for k in ids:
            soff.append(at)
            at += (k + 1) * 20
        buf = _aligned(at + GAP, FILL)
        buf[GAP: at] = 0  # the empty state: the caller clears the records
    else:
        buf, soff = into
    end = soff[-1] + (ids[-1] + 1) * 20
    tasks = []
    for i, img in enumerate(images):
        if i in skip:
            continue
        H, W = img.shape
        rows = run if run is not None else (1 if W >= HOST_RUN else HOST_RUN // W)
        y_lo, y_n = rows_of(i, H) if rows_of else (0, H)
        for y0 in range(y_lo, y_lo + y_n, rows):
            tasks.append(StatsTask(label_off=loff[i] + y0 * W * es, stat_off=soff[i], out_w=W, out_h=H, row0=y0,
                                   rows=min(rows, y_lo + y_n - y0), n_ids=ids[i], dtype=code))
    if spoil:
        spoil(tasks)
    n = len(tasks)
    arr = (StatsTask * max(n, 1))(*tasks)
    assert SL.launch("png_label_stats", arena, buf, arr, n, grid, emu=_emu) == 0
    assert (buf[:GAP] == FILL).all() and (buf[end:] == FILL).all(), "a sentinel around the records was written"
    assert arena.tobytes() == before.tobytes(), "the label arena was written"
    got = [buf[o: o + (k + 1) * 20].view(np.uint32).reshape(k + 1, 5).copy() for o, k in zip(soff, ids)]
    return got, tasks, (buf, soff)


def want(img, n_ids):
    return R.to_raw(R.stats_image(img, n_ids), img.shape[1], img.shape[0])


def check(images, n_ids, skip=(), **kw):
    got, tasks, _ = run(images, n_ids, skip=skip, **kw)
    ids = [n_ids] * len(images) if isinstance(n_ids, int) else list(n_ids)
    for i, (img, k) in enumerate(zip(images, ids)):
        exp = want(img, k) if i not in skip else np.zeros((k + 1, 5), np.uint32)
        assert got[i].dtype == exp.dtype and got[i].tobytes() == exp.tobytes(), (i, img.shape, k, kw.get("grid"), np.argwhere(got[i] != exp)[:4])
    return got, tasks


def _blocky(rng, H, W, n_ids, dtype, block=5):
    """rectangles of ids as a class map has them, "other" values among them"""
    small = rng.integers(0, n_ids + 2, (-(-H // block), -(-W // block)))
    img = np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:H, :W]
    return img.astype(dtype)


def _edge_values(name, n_ids):
    """the ends of the id range and the values outside it that the dtype can hold"""
    npdt = DTYPES[name][1]
    vals = [0, n_ids - 1, n_ids, 255, 65535]
    if name in ("int32", "int64"):
        vals += [-1, np.iinfo(npdt).min, np.iinfo(npdt).max]
    if name == "int64":
        vals += [2 ** 32 + 3, 2 ** 40, 2 ** 32, -2 ** 32 + 3]
    return [v for v in vals if np.iinfo(npdt).min <= v <= np.iinfo(npdt).max]


# ---- dtypes and sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(DTYPES))
def test_every_dtype_width_and_height(name):
    """all fifteen sizes of one dtype in one launch: blocky maps, and noise where the id changes at almost every element"""
    rng = np.random.default_rng(DTYPES[name][0])
    images = []
    for H in HEIGHTS:
        for W in WIDTHS:
            images.append(_blocky(rng, H, W, 21, DTYPES[name][1]))
            images.append(rng.integers(0, 23, (H, W)).astype(DTYPES[name][1]))
    _, tasks = check(images, 21)
    assert len(tasks) == len(images)
    check(images, 21, run=4, grid=3)


@pytest.mark.parametrize("name", list(DTYPES))
def test_runs_longer_than_one_round_of_the_lanes(name):
    """300 x 70: the host cuts 234 rows and 66 -- 16,380 elements, more than 256 items of every dtype, so every lane walks on to a
    next item (the add-and-compare of rows and columns), in front of an unaligned head and a tail"""
    rng = np.random.default_rng(7)
    img = _blocky(rng, 300, 70, 21, DTYPES[name][1], block=13)
    noise = rng.integers(0, 30, (300, 70)).astype(DTYPES[name][1])
    _, tasks = check([img, noise], 21)
    assert [t.rows for t in tasks] == [234, 66, 234, 66] and 234 * 70 // (16 // img.itemsize) > 256
    check([img, noise], 21, grid=1)


# ---- the id range ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ids", [1, 21, 256, 1024])
@pytest.mark.parametrize("name", list(DTYPES))
def test_the_ends_of_the_id_range(name, n_ids):
    npdt = DTYPES[name][1]
    vals = [v for v in _edge_values(name, n_ids)]
    rng = np.random.default_rng(n_ids)
    img = np.array(vals, dtype=npdt)[rng.integers(0, len(vals), (24, 33))]
    img[0, :len(vals)] = vals  # each of them at least once
    stripes = np.repeat(np.array(vals, dtype=npdt)[None, :], 5, axis=0)
    got, _ = check([img, stripes], n_ids)
    other = int((R.key_of(img, n_ids) == n_ids).sum())
    assert got[0][n_ids][0] == other and (other > 0) == any(not 0 <= v < n_ids for v in vals)
    assert other > 0 or (name, n_ids) in (("uint8", 256), ("uint8", 1024))  # (a uint8 holds nothing outside those ranges)
    if name == "int64":  # 2^32 + 3 is "other", never id 3
        assert 2 ** 32 + 3 in vals and (n_ids <= 3 or got[0][3][0] == 0)
    assert got[0][n_ids - 1][0] == (img == n_ids - 1).sum() and (got[0][n_ids - 1][0] > 0) == (n_ids - 1 in vals)


# ---- patterns --------------------------------------------------------------------------------------------------------------------------

def _patterns(npdt, H=24, W=33):
    flat = np.full((H, W), 7, npdt)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = ((yy + xx) % 2 * 3 + 2).astype(npdt)
    stripes = (xx % 2 + 4).astype(npdt)
    corners = np.full((H, W), 9, npdt)
    corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 10, 11, 12, 13
    last = np.full((H, W), 1, npdt)
    last[-1, -1] = 20
    seam = np.full((H, W), 3, npdt)  # with run=4: the last row of one task and the first row of the next
    seam[3, 5], seam[4, 30] = 15, 15
    return {"flat": flat, "checker": checker, "stripes": stripes, "corners": corners, "last": last, "seam": seam}


@pytest.mark.parametrize("name", list(DTYPES))
def test_patterns(name):
    P = _patterns(DTYPES[name][1])
    images = list(P.values())
    for kw in (dict(), dict(run=4), dict(run=1, grid=2)):
        got, _ = check(images, 21, **kw)
        g = dict(zip(P, got))
        assert g["flat"][7].tolist() == [24 * 33, 33, 24, 33, 24] and np.count_nonzero(g["flat"][:, 0]) == 1
        assert g["corners"][10].tolist() == [1, 1, 1, 33, 24] and g["corners"][13].tolist() == [1, 33, 24, 1, 1]
        assert g["corners"][11].tolist() == [1, 33, 1, 1, 24] and g["corners"][12].tolist() == [1, 1, 24, 33, 1]
        assert g["last"][20].tolist() == [1, 33, 24, 1, 1]
        assert g["seam"][15].tolist() == [2, 31, 5, 33 - 5, 24 - 3]


def test_flat_images_large_enough_for_every_wavefront():
    """one id over 16,380 elements: all 256 lanes close their records onto one entry, task after task"""
    for name in ("uint8", "int64"):
        img = np.full((300, 70), 5, DTYPES[name][1])
        got, _ = check([img, img], 6, grid=1)
        assert got[0][5].tolist() == [21000, 70, 300, 70, 300]


# ---- the task cut, the grid and the order ----------------------------------------------------------------------------------------------

def _transitions(tasks, n, grid, key):
    """[(kept, replaced)] per workgroup: how often its next task has the key of the one before / another"""
    out = []
    for wg in range(grid):
        held, kept, replaced = None, 0, 0
        for ti in range(wg, n, grid):
            k = key(tasks[ti])
            if held is not None:
                kept += k == held
                replaced += k != held
            held = k
        out.append((kept, replaced))
    return out


def _shuffled(seed):
    def spoil(tasks):
        rng = np.random.default_rng(seed)
        tasks[:] = [tasks[i] for i in rng.permutation(len(tasks))]
    return spoil


def _mixed(name):
    rng = np.random.default_rng(11)
    npdt = DTYPES[name][1]
    return [_blocky(rng, 24, 33, 21, npdt), rng.integers(0, 25, (24, 33)).astype(npdt), _blocky(rng, 5, 70, 21, npdt, block=3),
            np.full((24, 9), 2, npdt), _blocky(rng, 24, 70, 21, npdt, block=7)]


@pytest.mark.parametrize("name", ["uint8", "int64"])
def test_every_cut_grid_and_order_gives_the_same_records(name):
    images = _mixed(name)
    first = None
    for rows in (1, 4, None):
        for grid in (0, 1, 2, 3):
            for spoil in (None, _shuffled(grid + 1)):
                got, tasks = check(images, 21, run=rows, grid=grid, spoil=spoil)
                first = first or got
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
                if spoil is None and grid in (1, 2) and rows == 4:
                    assert len(tasks) > grid  # in image order one workgroup both keeps its table and replaces it
                    per_wg = _transitions(tasks, len(tasks), grid, lambda t: (t.stat_off, t.n_ids))
                    assert any(kept > 0 and replaced > 0 for kept, replaced in per_wg), per_wg


def test_tables_of_different_sizes_alternate_through_one_workgroup():
    """n_ids 300 and 5 in turn: "other" of the small table is entry 5 of the large one, and the large table's entries above 5 are
    beyond what the small image's flush clears -- a stale entry would show in the image behind"""
    rng = np.random.default_rng(3)
    big = [rng.integers(0, 310, (24, 33)).astype(np.int32) for _ in range(3)]
    small = [rng.integers(0, 8, (24, 33)).astype(np.int32) for _ in range(3)]
    images = [big[0], small[0], big[1], small[1], big[2], small[2]]
    ids = [300, 5] * 3
    for grid in (1, 2):  # (2: one workgroup takes the large tables only, the other the small ones)
        check(images, ids, run=24, grid=grid)
    _, tasks = check(images, ids, run=8, grid=1)
    assert _transitions(tasks, len(tasks), 1, lambda t: (t.stat_off, t.n_ids)) == [(12, 5)]
    # the same n_ids but another image: the record offset alone makes the workgroup flush
    check([small[0], small[1], small[0]], 5, run=8, grid=1)


# ---- skipped images and accumulation ---------------------------------------------------------------------------------------------------

def test_an_image_without_tasks_keeps_zero_records():
    images = _mixed("int32")
    got, tasks = check(images, 21, skip=(1, 4), run=4, grid=2)
    assert not got[1].any() and not got[4].any() and {t.stat_off for t in tasks} == {GAP, GAP + 2 * 22 * 20, GAP + 3 * 22 * 20}
    got, tasks = check(images, 21, skip=range(5))
    assert tasks == [] and not any(g.any() for g in got)


@pytest.mark.parametrize("grid", [0, 2])
def test_two_launches_over_two_halves_accumulate(grid):
    images = _mixed("uint16")
    whole, _, _ = run(images, 21, run=2, grid=grid)
    top, _, keep = run(images, 21, run=2, grid=grid, rows_of=lambda i, H: (0, H // 2))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(top, whole))
    both, _, _ = run(images, 21, run=2, grid=grid, rows_of=lambda i, H: (H // 2, H - H // 2), into=keep)
    for i, img in enumerate(images):
        assert both[i].tobytes() == whole[i].tobytes() == want(img, 21).tobytes(), i


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------

def test_tasks_that_break_a_bound_are_skipped():
    """every bound of include/debig_hip.h, one task each (and a good task between them, so that a table is held when they come):
    the bad tasks' records stay zero, the good task's are right, the sentinels stay"""
    rng = np.random.default_rng(5)
    images = [_blocky(rng, 24, 33, 21, np.int32) for _ in range(2)]

    def broken(field, value):
        def spoil(tasks):
            good = tasks[1]
            bad = StatsTask.from_buffer_copy(bytes(tasks[0]))
            setattr(bad, field, value(bad))
            tasks[:] = [bad, good, bad]
        return spoil

    cases = [("dtype", lambda t: 4), ("dtype", lambda t: 255), ("n_ids", lambda t: 0), ("n_ids", lambda t: 1025), ("n_ids", lambda t: 2 ** 32 - 1),
             ("out_w", lambda t: 0), ("out_w", lambda t: 16385), ("out_h", lambda t: 0), ("out_h", lambda t: 16385), ("rows", lambda t: 0),
             ("rows", lambda t: 25), ("row0", lambda t: 1), ("row0", lambda t: 24), ("row0", lambda t: 2 ** 32 - 1), ("rows", lambda t: 2 ** 32 - 1),
             ("stat_off", lambda t: t.stat_off + 2), ("stat_off", lambda t: t.stat_off + 1), ("label_off", lambda t: t.label_off + 1),
             ("label_off", lambda t: t.label_off + 2)]
    for field, value in cases:
        for grid in (0, 1):
            got, tasks, _ = run(images, 21, run=24, grid=grid, spoil=broken(field, value))
            assert len(tasks) == 3
            assert not got[0].any(), (field, value(tasks[1]), grid)
            assert got[1].tobytes() == want(images[1], 21).tobytes(), (field, grid)
    # (the int64 twin of the offset rule: 4 is a multiple of int32 but not of the element)
    im64 = [im.astype(np.int64) for im in images]
    got, _, _ = run(im64, 21, run=24, grid=1, spoil=broken("label_off", lambda t: t.label_off + 4))
    assert not got[0].any() and got[1].tobytes() == want(im64[1], 21).tobytes()
