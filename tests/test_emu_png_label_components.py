"""The five label-components kernels (csrc/png_label_components_kernel.inc) on the CPU lock-step emulator against the numpy
restatement tests/png_label_components_ref.py (a fixpoint of minima; no trees, no unions):
  * run() lays the images out one behind the other -- labels, parent planes and outputs each starting at a byte that is NOT a
    multiple of 16 -- cuts each image into runs of rows and launches rows, merge, count, number (CONSECUTIVE) and finish through
    tests/stage_launch.py.  The parent arena, the counts and the output lie between two sentinels of 4 KiB and are filled with a
    pattern before the first launch, so a byte that no task owns must keep it; the label arena must come back unchanged, and the
    launches after merge must leave the parent arena unchanged;
  * the plane after merge is NOT a pure function of the input (it depends on the order of the unions), so its INVARIANTS are
    checked: a background slot holds 0xffffffff, every other slot an index that is not above its own, and a host-side find from
    every element ends at the restatement's FIRST.  Every task's count after the count launch, and every byte of the final output
    in both id modes, are compared with the restatement.
THE EMULATOR RUNS THE WORKGROUPS ONE AFTER THE OTHER: this battery proves the rule, the cut and the bounds, not the races between
workgroups on one plane.  tests/test_gpu_png_label_components.py runs it as it is on the GPU, which is what exercises the races."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_components_ref as R  # noqa: E402
import stage_launch as SL  # noqa: E402
from emu_binding import load_emu  # noqa: E402

FILL, GAP = 0xEE, 4096
DTYPES = {"uint8": (0, np.uint8), "uint16": (1, np.uint16), "int32": (2, np.int32), "int64": (3, np.int64)}  # DEBIG_PNG_L_*
ELEMS = 16384  # include/debig_hip.h: DEBIG_PNG_LABEL_COMPONENTS_ELEMS
HEIGHTS = [1, 2, 3, 5, 17, 40]
IDS = {"first": 0, "consecutive": 1}
BG = 0xFFFFFFFF
ROWS, MERGE, COUNT, NUMBER, FINISH = ("png_label_components_" + s for s in ("rows", "merge", "count", "number", "finish"))
KERNELS = {ROWS: (SL.IN, SL.OUT, SL.TASKS), MERGE: (SL.IN, SL.INOUT, SL.TASKS), COUNT: (SL.IN, SL.OUT, SL.TASKS),
           NUMBER: (SL.IN, SL.IN, SL.OUT, SL.TASKS), FINISH: (SL.IN, SL.INOUT, SL.TASKS)}


class Task(C.Structure):  # include/debig_hip.h: debig_png_label_components_task
    _fields_ = [("label_off", C.c_uint64), ("parent_off", C.c_uint64), ("out_off", C.c_uint64), ("background", C.c_int64),
                ("w", C.c_uint32), ("h", C.c_uint32), ("row0", C.c_uint32), ("rows", C.c_uint32), ("dtype", C.c_uint32),
                ("connectivity", C.c_uint32), ("use_background", C.c_uint32), ("ids", C.c_uint32), ("count_idx", C.c_uint32),
                ("count_first", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(Task) == 80
_LIB = {}
_REF = {}  # the restatement of an image, computed once: (the image's values, its shape, connectivity, background) -> FIRST, never changed


def _emu():
    if "L" not in _LIB:
        L = load_emu()
        for name, roles in KERNELS.items():
            fn = getattr(L, "emu_%s_batch" % name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p] * len(roles) + [C.c_uint32, C.c_uint32]
        _LIB["L"] = L
    return _LIB["L"]


@pytest.fixture(autouse=True)
def the_launchers_are_known(monkeypatch):
    """tests/stage_launch.py learns the five launchers for the length of one test (its table is another test's yardstick)"""
    for name, roles in KERNELS.items():
        monkeypatch.setitem(SL.KERNELS, name, roles)


def _aligned(n, fill):
    """n bytes of `fill` that start at a multiple of 64 (a view: the launch seam keeps the address's residue on the GPU)"""
    root = np.full(n + 64, fill, np.uint8)
    off = -root.ctypes.data % 64
    return root[off: off + n]


def ref(img, connectivity, background):
    whole = R._whole(img).astype(np.int64)
    if background is not None and not np.iinfo(R._whole(img).dtype).min <= background <= np.iinfo(R._whole(img).dtype).max:
        background = None  # nothing equals it
    key = (whole.tobytes(), whole.shape, connectivity, background)
    if key not in _REF:
        _REF[key] = R.first(whole, connectivity, background)
    return _REF[key]


def host_run(W):
    """the rows of one task as debig_png_label_components cuts them"""
    return 1 if W >= ELEMS else ELEMS // W


def _launch(name, bufs, tasks, grid):
    assert SL.launch(name, *bufs, (Task * max(len(tasks), 1))(*tasks), len(tasks), grid, emu=_emu) == 0


def run(images, connectivity=4, background=None, ids="first", rows=None, grid=0, skip=(), spoil=None, keep_finish=None, corrupt=None):
    """images: (H, W) arrays of one dtype; rows: the rows of a task (None: the host's cut); skip: images that get no task;
    spoil(tasks, owned): edits the list; keep_finish(k, task) -> False drops a task from the finish launch; corrupt(plane bytes of
    the arena, a view): edits the parent arena between rows and merge
    -> ([parent plane (H, W) uint32 per image after merge], counts uint32 per count word, [output (H, W) int32 per image], tasks,
        [bool (H,): rows owned by a task], [bool (H,): rows owned by a finish task], the planes' offsets)"""
    code, npdt = next(v for v in DTYPES.values() if v[1] == images[0].dtype)
    es = np.dtype(npdt).itemsize
    loff, poff, ooff, at, pt, ot = [], [], [], 0, GAP, GAP
    for img in images:  # every image, parent plane and output image starts one element behind a multiple of 16 bytes
        at += -at % 16 + es
        loff.append(at)
        at += img.size * es
        pt += -pt % 16 + 4
        poff.append(pt)
        pt += img.size * 4
        ot += -ot % 16 + 4
        ooff.append(ot)
        ot += img.size * 4
    arena = _aligned(at, 0x5A)
    for img, o in zip(images, loff):
        assert o % 16 != 0 and arena[o:].ctypes.data % 16 != 0
        arena[o: o + img.size * es] = np.ascontiguousarray(img).reshape(-1).view(np.uint8)
    before = arena.copy()
    tasks, owned, n_words = [], [np.zeros(img.shape[0], bool) for img in images], 0
    for i, img in enumerate(images):
        if i in skip:
            continue
        H, W = img.shape
        per = rows or host_run(W)
        first_word = n_words
        for y0 in range(0, H, per):
            tasks.append(Task(label_off=loff[i], parent_off=poff[i], out_off=ooff[i], background=0 if background is None else background,
                              w=W, h=H, row0=y0, rows=min(per, H - y0), dtype=code, connectivity=connectivity,
                              use_background=0 if background is None else 1, ids=IDS[ids], count_idx=n_words, count_first=first_word))
            n_words += 1
            owned[i][y0: y0 + per] = True
    n_words += 3  # (words that no task has)
    if spoil:
        spoil(tasks, owned)
    pbuf, cfull, obuf = _aligned(pt + GAP, FILL), _aligned(2 * GAP + 4 + n_words * 4, FILL), _aligned(ot + GAP, FILL)
    cbuf = cfull[GAP + 4:]  # the counts start 4 bytes behind a multiple of 16

    def guards(what):
        assert arena.tobytes() == before.tobytes(), (what, "the label arena was written")
        assert (pbuf[:GAP] == FILL).all() and (pbuf[pt:] == FILL).all(), (what, "a sentinel around the parent planes was written")
        assert (cfull[:GAP + 4] == FILL).all() and (cbuf[n_words * 4:] == FILL).all(), (what, "a sentinel around the counts was written")
        assert (obuf[:GAP] == FILL).all() and (obuf[ot:] == FILL).all(), (what, "a sentinel around the output was written")
        p_at, o_at = GAP, GAP
        for img, po, oo in zip(images, poff, ooff):
            assert (pbuf[p_at: po] == FILL).all(), (what, "the bytes between two parent planes were written")
            assert (obuf[o_at: oo] == FILL).all(), (what, "the bytes between two output images were written")
            p_at, o_at = po + img.size * 4, oo + img.size * 4

    _launch(ROWS, (arena, pbuf), tasks, grid)
    guards("rows")
    if corrupt:
        corrupt(pbuf, poff)
    _launch(MERGE, (arena, pbuf), tasks, grid)
    guards("merge")
    planes = [pbuf[o: o + img.size * 4].view(np.uint32).reshape(img.shape).copy() for img, o in zip(images, poff)]
    pbefore = pbuf.copy()
    _launch(COUNT, (pbuf, cbuf), tasks, grid)
    counts = cbuf[: n_words * 4].view(np.uint32).copy()
    if ids == "consecutive":
        _launch(NUMBER, (pbuf, cbuf, obuf), tasks, grid)
    fin = [t for k, t in enumerate(tasks) if keep_finish is None or keep_finish(k, t)]
    fowned = [o.copy() for o in owned]
    if keep_finish is not None:
        for o in fowned:
            o[:] = False
        for t in fin:
            i = poff.index(t.parent_off)
            fowned[i][t.row0: t.row0 + t.rows] = True
    _launch(FINISH, (pbuf, obuf), fin, grid)
    guards("finish")
    assert pbuf.tobytes() == pbefore.tobytes(), "a launch after merge wrote the parent planes"
    assert cbuf[: n_words * 4].view(np.uint32).tobytes() == counts.tobytes(), "a launch after count wrote the counts"
    got = [obuf[o: o + img.size * 4].view(np.int32).reshape(img.shape).copy() for img, o in zip(images, ooff)]
    return planes, counts, got, tasks, owned, fowned, poff


def host_find(plane):
    """the root above every element of a plane whose slots are not above their own index (background: itself)"""
    flat = plane.reshape(-1).astype(np.int64)
    idx = np.arange(flat.size)
    link = np.where(flat == BG, idx, flat)
    r = idx.copy()
    for _ in range(flat.size + 1):
        nr = link[r]
        if np.array_equal(nr, r):
            return r.reshape(plane.shape)
        r = nr
    raise AssertionError("a cycle in the parent plane")


def check(images, connectivity=4, background=None, ids="first", skip=(), **kw):
    planes, counts, got, tasks, owned, fowned, poff = run(images, connectivity, background, ids, skip=skip, **kw)
    pattern32 = np.frombuffer(bytes([FILL]) * 4, np.uint32)[0]
    counted = np.zeros(counts.size, bool)
    for i, img in enumerate(images):
        H, W = img.shape
        fst = ref(img, connectivity, background)
        idx = np.arange(H * W).reshape(H, W)
        own = owned[i][:, None] & np.ones((1, W), bool)
        # the plane's invariants (complete only when the whole image was merged)
        plane = planes[i]
        assert (plane[~own] == pattern32).all(), (i, "a slot that no task owns was written")
        if owned[i].all():
            back = fst < 0
            assert (plane[back] == BG).all() and (plane[~back] <= idx[~back]).all(), (i, img.shape, "the plane's invariants")
            roots = host_find(plane)
            assert np.array_equal(roots[~back], fst[~back]), (i, img.shape, connectivity, background, np.argwhere(roots != np.where(back, idx, fst))[:4])
        want = fst if ids == "first" else R.consecutive(fst)[0]
        exp = np.where(fowned[i][:, None], want, pattern32.view(np.int32))
        if ids == "consecutive":  # the roots are numbered by the number launch, whose tasks are all there
            exp = np.where(own & (fst == idx), want, exp)
        assert got[i].tobytes() == exp.astype(np.int32).tobytes(), (i, img.shape, connectivity, background, ids, kw.get("rows"), kw.get("grid"),
                                                                    np.argwhere(got[i] != exp)[:4])
    # every task's count
    for t in tasks:
        i = poff.index(t.parent_off) if t.parent_off in poff else None
        if i is None or not owned[i].all():  # (a task that breaks a bound: its image is not owned)
            continue
        fst = ref(images[i], connectivity, background)
        W = images[i].shape[1]
        rows_first = (fst[t.row0: t.row0 + t.rows] == np.arange(t.row0 * W, (t.row0 + t.rows) * W).reshape(-1, W)).sum()
        assert counts[t.count_idx] == rows_first, (i, t.row0, t.rows, counts[t.count_idx], rows_first)
        counted[t.count_idx] = True
    assert (counts[~counted] == pattern32).all(), "a count that no task owns was written"
    return got, tasks


def _blocky(rng, H, W, dtype, block=5, ids=4):
    small = rng.integers(0, ids, (-(-H // block), -(-W // block)))
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:H, :W].astype(dtype)


def _absent_and_unholdable(name):
    """a value that no map below holds, and one the dtype cannot hold whose low bits are a value the maps do hold (int64 holds
    every value the task can carry: another absent one)"""
    return 77, {"uint8": 256 + 1, "uint16": 65536 + 1, "int32": 2 ** 32 + 1, "int64": -(2 ** 63)}[name]


# ---- dtypes and sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(DTYPES))
def test_every_dtype_width_height_and_background(name, connectivity):
    """widths 1 .. 70 x six heights: blocky maps under the host's cut with no background, a present one, an absent one and one the
    dtype cannot hold; noise in runs of 3 rows with three workgroups.  The maps are the same for every dtype: the restatement is
    computed once"""
    rng = np.random.default_rng(7)
    npdt = DTYPES[name][1]
    blocky = [_blocky(rng, H, W, npdt) for i, W in enumerate(range(1, 71)) for H in (HEIGHTS[i % 6], HEIGHTS[(i + 3) % 6])]
    noise = [rng.integers(0, 3, (HEIGHTS[(i + 1) % 6], W)).astype(npdt) for i, W in enumerate(range(1, 71))]
    absent, unholdable = _absent_and_unholdable(name)
    for k, background in enumerate((None, 1, absent, unholdable)):
        _, tasks = check(blocky, connectivity, background, ("first", "consecutive")[k % 2])
        assert len(tasks) == len(blocky)
        check(noise, connectivity, background, ("consecutive", "first")[k % 2], rows=3, grid=3)


def test_flat_images_and_images_that_are_all_background():
    flat = [np.full((5, 70), 7, np.uint8), np.full((40, 3), 7, np.uint8), np.full((1, 1), 7, np.uint8)]
    for connectivity in (4, 8):
        for ids in IDS:
            got, _ = check(flat, connectivity, None, ids, rows=2)
            assert all((g == (0 if ids == "first" else 1)).all() for g in got)
            got, _ = check(flat, connectivity, 7, ids, rows=2)
            assert all((g == (-1 if ids == "first" else 0)).all() for g in got)
            got, _ = check(flat, connectivity, 7 + 256, ids)
            assert all((g == (0 if ids == "first" else 1)).all() for g in got)


# ---- shapes that tell the rules apart ------------------------------------------------------------------------------------------------------

def test_a_checkerboard_is_every_element_under_4_and_two_components_under_8():
    yy, xx = np.mgrid[0:17, 0:23]
    board = ((yy + xx) % 2).astype(np.uint16)
    got, _ = check([board], 4, None, "consecutive", rows=4)
    assert np.array_equal(got[0], np.arange(1, 17 * 23 + 1).reshape(17, 23))
    got, _ = check([board], 8, None, "consecutive", rows=4)
    assert np.array_equal(got[0], board + 1)
    got, _ = check([board], 8, 0, "first", rows=1)
    assert np.array_equal(got[0], np.where(board == 1, 1, -1))


def test_diagonal_lines_tell_4_from_8():
    H, W = 24, 31
    yy, xx = np.mgrid[0:H, 0:W]
    for img in (((yy - xx) % 5 == 0), ((yy + xx) % 5 == 0), ((yy - xx) % 5 == 0) | ((yy + xx) % 7 == 0)):
        img = img.astype(np.int32)
        g4, _ = check([img], 4, 0, "consecutive", rows=5)
        g8, _ = check([img], 8, 0, "consecutive", rows=5)
        assert g4[0].max() > g8[0].max() >= 1
        check([img], 8, None, "first", rows=1)


def _comb(H, W, up):
    """arms of ones, one column apart, that meet only in the last (up: the first) row"""
    img = np.zeros((H, W), np.uint8)
    img[:, ::2] = 1
    img[0 if up else H - 1, :] = 1
    return img


def _spiral(n):
    """a square spiral of ones, one element wide, walls of zeros one element wide: one component of ones"""
    img = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    img[0, 0] = 1
    while True:
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny < n and 0 <= nx < n and img[ny, nx] == 0
        beyond = not (0 <= ny + dy < n and 0 <= nx + dx < n) or img[ny + dy, nx + dx] == 0
        if ahead and beyond:
            y, x = ny, nx
            img[y, x] = 1
            continue
        dy, dx = dx, -dy  # turn right
        ny, nx = y + dy, x + dx
        if not (0 <= ny < n and 0 <= nx < n and img[ny, nx] == 0) or (0 <= ny + dy < n and 0 <= nx + dx < n and img[ny + dy, nx + dx] == 1):
            return img
        y, x = ny, nx
        img[y, x] = 1


def _serpentine(H, W):
    """corridors of ones in every other row, joined at alternating ends: one component of ones"""
    img = np.zeros((H, W), np.uint8)
    img[::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        img[y, W - 1 if k % 2 == 0 else 0] = 1
    return img


@pytest.mark.parametrize("rows", [None, 1, 3])
def test_trees_that_merge_late(rows):
    """U, comb and spiral: arms whose trees have grown on their own before the last row joins them; a serpentine: one long chain"""
    u = np.zeros((17, 9), np.uint8)
    u[:, 0] = u[:, 8] = u[16, :] = 1
    imgs = [u, u[::-1].copy(), _comb(17, 31, False), _comb(17, 31, True), _spiral(29), _spiral(30), _serpentine(21, 13), _serpentine(40, 70).T.copy()]
    for connectivity in (4, 8):
        got, _ = check(imgs, connectivity, 0, "consecutive", rows=rows, grid=0 if rows is None else 2)
        assert all(g.max() == 1 for g in got)
        check(imgs, connectivity, None, "first", rows=rows)


def test_concentric_rings_and_vertical_bars():
    yy, xx = np.mgrid[0:33, 0:41]
    rings = (np.maximum(abs(yy - 16), abs(xx - 20)) % 2).astype(np.int64)
    bars = (xx % 2).astype(np.int64)
    for connectivity in (4, 8):
        got, _ = check([rings, bars], connectivity, None, "consecutive", rows=4)
        assert got[0].max() == 17 + 2 * 4 and got[1].max() == 41  # 17 whole rings, four that the image cuts in two
        check([rings, bars], connectivity, 1, "first", rows=7, grid=3)


def test_equal_values_that_touch_only_at_a_corner():
    img = np.array([[5, 0, 0, 5],
                    [0, 5, 5, 0],
                    [0, 5, 0, 5],
                    [5, 0, 5, 0]], np.uint8)
    g4, _ = check([img], 4, 0, "consecutive", rows=1)
    g8, _ = check([img], 8, 0, "consecutive", rows=1)
    assert g4[0].tolist() == [[1, 0, 0, 2], [0, 3, 3, 0], [0, 3, 0, 4], [5, 0, 6, 0]]
    assert g8[0].tolist() == [[1, 0, 0, 1], [0, 1, 1, 0], [0, 1, 0, 1], [1, 0, 1, 0]]
    g8n, _ = check([img], 8, None, "consecutive")
    assert g8n[0].tolist() == [[1, 2, 2, 1], [2, 1, 1, 2], [2, 1, 2, 1], [1, 2, 1, 2]]


def test_elements_are_compared_whole():
    a = np.full((9, 9), 3, np.int64)
    a[4:, :] = 2 ** 32 + 3  # the low word is equal: they must not join
    a[0, 0] = -1
    got, _ = check([a], 8, None, "consecutive", rows=2)
    assert got[0].max() == 3 and got[0][0, 0] == 1 and got[0][0, 1] == 2 and (got[0][4:] == 3).all()
    got, _ = check([a], 4, 3, "consecutive")  # the background 3 is not 2^32 + 3
    assert (got[0][4:] == 2).all() and (got[0][1:4] == 0).all()
    b = np.full((5, 7), -1, np.int32)
    b[2, :] = 255
    got, _ = check([b], 4, 255, "consecutive")
    assert got[0].max() == 2 and (got[0][2] == 0).all()
    got, _ = check([b], 4, -1, "consecutive")
    assert got[0].max() == 1 and (got[0][2] == 1).all()
    got, _ = check([b], 4, 2 ** 32 - 1, "consecutive")  # int32 cannot hold it, though -1 has its bits
    assert got[0].max() == 3
    c = np.full((5, 7), 0xFFFF, np.uint16)
    c[:, 3] = 0x00FF
    got, _ = check([c], 8, 0xFFFF, "first")
    assert (got[0][:, 3] == 3).all() and (np.delete(got[0], 3, axis=1) == -1).all()
    got, _ = check([c], 8, -1, "consecutive")  # uint16 cannot hold -1
    assert got[0].max() == 3


# ---- the cut, the grid and the order -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uint8", "int64"])
def test_row_runs_cut_at_every_seam(name):
    """70 x 40: every run of rows 1 .. 40 gives the bytes of the host's cut"""
    rng = np.random.default_rng(12)
    npdt = DTYPES[name][1]
    imgs = [_blocky(rng, 40, 70, npdt, block=9), rng.integers(0, 2, (40, 70)).astype(npdt), _spiral(40).astype(npdt)]
    firsts = {}
    for rows in range(1, 41):
        connectivity, ids = (4, 8)[rows % 2], ("first", "consecutive")[(rows // 2) % 2]
        got, tasks = check(imgs, connectivity, (None, 0)[(rows // 4) % 2], ids, rows=rows, grid=rows % 4)
        assert len(tasks) == 3 * -(-40 // rows)
        key = (connectivity, ids, (rows // 4) % 2)
        firsts.setdefault(key, got)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, firsts[key]))


def _mixed(name):
    rng = np.random.default_rng(11)
    npdt = DTYPES[name][1]
    return [_blocky(rng, 24, 33, npdt), rng.integers(0, 2, (24, 33)).astype(npdt), _blocky(rng, 5, 70, npdt, block=3),
            np.full((24, 9), 2, npdt), _serpentine(40, 70).astype(npdt)]


def _order(kind):
    def spoil(tasks, owned):
        if kind == "reversed":
            tasks.reverse()
        else:
            rng = np.random.default_rng(5)
            tasks[:] = [tasks[i] for i in rng.permutation(len(tasks))]
    return spoil


@pytest.mark.parametrize("name", ["uint16", "int32"])
def test_fewer_workgroups_than_tasks_in_both_orders(name):
    images = _mixed(name)
    first = None
    for grid in (0, 1, 2, 5):
        for spoil in (None, _order("reversed"), _order("shuffled")):
            got, tasks = check(images, 8, None, "consecutive", rows=7, grid=grid, spoil=spoil)
            first = first or got
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
            assert len(tasks) > 10
    check(images, 4, 2, "first", rows=7, grid=2, spoil=_order("reversed"))


def test_a_finish_launch_over_half_the_tasks_writes_only_those():
    images = _mixed("uint8")
    got, tasks = check(images, 4, None, "first", rows=3, keep_finish=lambda k, t: k % 2 == 0, grid=2)
    assert len(tasks) > 10 and any((g.view(np.uint8) == FILL).all(axis=1).any() for g in got)


def test_images_without_tasks_keep_the_pattern():
    images = _mixed("uint16")
    got, tasks = check(images, 8, 0, "consecutive", skip=(1, 4), rows=5, grid=2)
    assert (got[1].view(np.uint8) == FILL).all() and (got[4].view(np.uint8) == FILL).all() and tasks
    got, tasks = check(images, 4, None, "first", skip=range(5))
    assert tasks == [] and all((g.view(np.uint8) == FILL).all() for g in got)


# ---- the long shapes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 16384), (16384, 1), (3, 5000)])
def test_long_shapes(shape):
    """1 x 16384: the row scan's carries over 256 segments, one run over all of them; 16384 x 1: one task whose lanes hang 16384
    elements below each other; 3 x 5000: a task of the largest run of rows that fits"""
    rng = np.random.default_rng(shape[1])
    flat = np.zeros(shape, np.uint8)
    runs = np.repeat(rng.integers(0, 2, -(-flat.size // 37)), 37)[: flat.size].reshape(shape).astype(np.uint8)
    noise = rng.integers(0, 2, shape).astype(np.uint8)
    for img in (flat, runs, noise):
        got, _ = check([img], 4, None, "consecutive")
        check([img], 8, 1, "first")
    assert got[0].max() > 1000
    if shape == (3, 5000):
        check([noise], 8, None, "consecutive", rows=2)


# ---- the bounds (emulator only) ------------------------------------------------------------------------------------------------------------

def test_tasks_that_break_a_bound_are_skipped():
    """every bound of include/debig_hip.h, one task each, between good tasks, through all five launches: what the bad task owns
    keeps the pattern, the good tasks' elements are right, the sentinels stay"""
    rng = np.random.default_rng(5)
    images = [_blocky(rng, 24, 33, np.int32), _blocky(rng, 24, 33, np.int32)]

    def broken(field, value):
        def spoil(tasks, owned):
            bad = Task.from_buffer_copy(bytes(tasks[0]))
            setattr(bad, field, value(bad))
            tasks[:] = [bad, tasks[1], bad]
            owned[0][:] = False
        return spoil

    cases = [("dtype", lambda t: 4), ("dtype", lambda t: 2 ** 31), ("connectivity", lambda t: 0), ("connectivity", lambda t: 6),
             ("connectivity", lambda t: 12), ("connectivity", lambda t: 2 ** 32 - 4), ("use_background", lambda t: 2), ("ids", lambda t: 2),
             ("ids", lambda t: 2 ** 31), ("w", lambda t: 0), ("w", lambda t: 16385), ("h", lambda t: 0), ("h", lambda t: 16385),
             ("rows", lambda t: 0), ("rows", lambda t: 25), ("row0", lambda t: 24), ("row0", lambda t: 1), ("row0", lambda t: 2 ** 32 - 1),
             ("rows", lambda t: 2 ** 32 - 1), ("label_off", lambda t: t.label_off + 1), ("label_off", lambda t: t.label_off + 2),
             ("parent_off", lambda t: t.parent_off + 1), ("parent_off", lambda t: t.parent_off + 2), ("out_off", lambda t: t.out_off + 1),
             ("out_off", lambda t: t.out_off + 2), ("count_first", lambda t: t.count_idx + 1), ("count_idx", lambda t: t.count_first + 16384)]
    for field, value in cases:
        for grid in (0, 1):
            _, tasks = check(images, 8, 1, "consecutive", rows=24, grid=grid, spoil=broken(field, value))
            assert len(tasks) == 3
    # a run of more than 16384 elements in more than one row
    wide = [np.zeros((4, 5000), np.uint8), np.zeros((4, 5000), np.uint8)]
    wide[1][2, 77] = 1
    def none_owned(tasks, owned):
        owned[0][:] = owned[1][:] = False

    _, tasks = check(wide, 4, None, "consecutive", rows=4, spoil=none_owned)
    assert len(tasks) == 2 and tasks[0].rows == 4
    check(wide, 4, None, "consecutive", rows=3)


def test_a_corrupted_parent_plane_ends_cleanly():
    """a plane that the rows launch did not write: indices outside the image, above their slot, and whatever else 32 bits hold.
    Every launch behind it ends, and writes nothing outside the planes, the counts and the outputs (the stand-alone sanitizer
    program, tools/asan_png_label_components_emu.cpp, shows the same for the reads)"""
    rng = np.random.default_rng(9)
    images = [_blocky(rng, 24, 33, np.uint8), rng.integers(0, 2, (17, 70)).astype(np.uint8)]
    for kind in range(4):
        def corrupt(pbuf, poff):
            for img, o in zip(images, poff):
                plane = pbuf[o: o + img.size * 4].view(np.uint32)
                n = img.size
                plane[:] = [rng.integers(0, 2 ** 32, n), np.arange(n) + 1 + rng.integers(0, 5, n), np.full(n, n), rng.integers(0, n, n)][kind]
        for connectivity in (4, 8):
            for ids in IDS:
                run(images, connectivity, None, ids, rows=5, grid=2, corrupt=corrupt)
