"""The four kernels of the elastic deformation (csrc/png_elastic_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the
numpy restatement tests/png_elastic_ref.py.  The runners, sources, crops, output sizes, arenas and sentinels are those of the warp
batteries (test_emu_png_warp, test_emu_png_color, test_emu_png_color_labels_warp): tests/map_launch.py extends their tasks by
the field words and launches the elastic twin, so the shapes are the smallest at which these kernels go wrong --
  * crops of 1 x 1, 1 x 9 and 13 x 7 inside a larger image at odd arena offsets; output widths 1, 7, 64, 65 and 257; task runs that
    do not divide out_h; fewer workgroups than tasks; channels 1 - 4, P = 8 / 16, all dtypes, both layouts, filters and borders;
  * grids of 2 x 2, 3 x 5 and 33 x 33 nodes (more cells than pixels on the small outputs);
  * labels of 1 and 2 bytes with and without a LUT; colour labels in PACK and MAP with `unmatched` compared; the colour matrix.
The fields (fields() below): smooth random ones of a few pixels, a field of zeros, no field (UINT64_MAX), nodes alternating between
+2^28 and -2^28 (the limit), and a constant field.  Within one launch consecutive jobs name different fields, so a workgroup
re-stages its grid between tasks; with one workgroup (grid = 1) it alternates between two files' fields task by task.  Tasks that
break a bound are skipped with the sentinels intact (emulator only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_launch as EL  # noqa: E402
import png_elastic_ref as ER  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_emu_png_color as EC  # noqa: E402
import test_emu_png_color_labels_warp as ECL  # noqa: E402
import test_emu_png_warp as EW  # noqa: E402

FILL = EW.FILL
BOXES, SIZES = EW.BOXES, EW.SIZES
GRIDS = [(2, 2), (3, 5), (33, 33)]  # (grid_h, grid_w)
LIMIT = 1 << 28
SOME = ("identity", "rot90", "shift partly outside", "30 degrees, scale 0.7", "zoom 40", "linear entries 32768", "translation -2^24")


# ---- the matrices and the fields ---------------------------------------------------------------------------------------------------

def matrices(cw, chh, size, names=SOME):
    ms = EW.matrices(cw, chh, size)
    return {k: ms[k] for k in names}


def smooth(grid, seed, amp=3.0):
    """a random field of up to `amp` output pixels, quantised"""
    rng = np.random.default_rng(seed)
    return ER.quantise_field(rng.uniform(-amp, amp, size=(grid[0], grid[1], 2)))


def at_the_limit(grid, sign=1):
    gh, gw = grid
    yy, xx = np.mgrid[0:gh, 0:gw]
    s = sign * np.where((yy + xx) % 2 == 0, LIMIT, -LIMIT)
    return np.stack([s, -s], axis=2).astype(np.int64)


def fields(grid, n, seed=0):
    """n fields for n consecutive jobs: no two neighbours are the same object, every kind occurs when n >= 5"""
    kinds = [lambda k: smooth(grid, seed + k), lambda k: None, lambda k: at_the_limit(grid), lambda k: smooth(grid, seed + k, 40.0),
             lambda k: np.zeros(grid + (2,), np.int64), lambda k: np.broadcast_to(np.array([3 << 16, -(2 << 16)]), grid + (2,)).copy()]
    return [kinds[k % len(kinds)](k) for k in range(n)]


def test_the_special_fields_hit_what_they_are_for():
    for grid in GRIDS:
        assert np.abs(at_the_limit(grid)).max() == LIMIT
        # next to the edge nodes the displacement comes close to the limit, with both signs, and stays below 2^29
        Dx, Dy = ER.displacement((40, 65), at_the_limit(grid))
        assert LIMIT * 9 // 10 < int(Dx.max()) < 1 << 29 and LIMIT * 9 // 10 < int(-Dx.min()) < 1 << 29
    # (c) a 4 x 4 output under a 9 x 9 grid: every pixel centre lies on node (2Y + 1, 2X + 1)
    q9 = smooth((9, 9), 5)
    Dx, Dy = ER.displacement((4, 4), q9)
    assert np.array_equal(Dx, q9[1::2, 1::2, 0]) and np.array_equal(Dy, q9[1::2, 1::2, 1])
    # zeros and None are the affine rule; a constant field of whole pixels is a translation
    size, m = (5, 65), EW.matrices(13, 7, (5, 65))["30 degrees, scale 0.7"]
    for qf in (None, np.zeros((3, 5, 2), np.int64)):
        assert all(np.array_equal(x, y) for x, y in zip(ER.positions(size, m, qf), WR.positions(size, m)))
    const = np.broadcast_to(np.array([3 << 16, -(2 << 16)]), (3, 5, 2))
    moved = list(m)
    moved[2] += 3 * m[0] - 2 * m[1]
    moved[5] += 3 * m[3] - 2 * m[4]
    assert all(np.array_equal(x, y) for x, y in zip(ER.positions(size, m, const), WR.positions(size, moved)))


# ---- the runners of the warp batteries, through the elastic kernels ---------------------------------------------------------------

def run_elastic(srcs, jobs, size, nodes, *a, **kw):
    """jobs: [(source index, box, m6, q)] -> EW.run_warp's result from debig_png_elastic_kernel"""
    with EL.as_elastic(EW, [j[3] for j in jobs], nodes):
        return EW.run_warp(srcs, [(si, box, m) for si, box, m, _ in jobs], size, *a, **kw)


def run_label_elastic(srcs, jobs, size, nodes, *a, **kw):
    with EL.as_elastic(EW, [j[3] for j in jobs], nodes):
        return EW.run_label_warp(srcs, [(si, box, m) for si, box, m, _ in jobs], size, *a, **kw)


def run_color_label_elastic(srcs, jobs, size, nodes, *a, **kw):
    """jobs: [(source index, box, map index, m6, q)]"""
    with EL.as_elastic(ECL, [j[4] for j in jobs], nodes):
        return ECL.run_warp(srcs, [(si, box, mi, m) for si, box, mi, m, _ in jobs], size, *a, **kw)


def run_elastic_color(srcs, mats, ms, qs, size, nodes, *a, **kw):
    with EL.as_elastic(EC, qs, nodes):
        return EC.run_warp(srcs, mats, ms, size, *a, **kw)


# ---- the image kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_elastic_format_grid(ch, P):
    """every dtype x layout x filter x border mode, each on every matrix and field kind; crops, sizes and grids rotate"""
    src = EW._source(ch, P)
    border = [(1 << P) - 1, 0, 77, 1 << (P - 1)]
    k = 0
    for dtype in Z.DTYPES:
        for layout in ("hwc", "chw"):
            for filt in (WR.BILINEAR, WR.NEAREST):
                for mode in (WR.CONSTANT, WR.CLAMP):
                    size, box, grid = SIZES[(k + k // 5) % len(SIZES)], BOXES[k % len(BOXES)], GRIDS[k % len(GRIDS)]
                    k += 1
                    ms = matrices(box[2], box[3], size)
                    qs = fields(grid, len(ms), seed=k)
                    got = run_elastic([src], [(0, box, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, dtype, layout, filt, mode,
                                      border, run=3 if size[0] > 3 else None, grid=0 if k % 3 else 4)
                    for j, name in enumerate(ms):
                        exp = ER.warp(src, size, ms[name], qs[j], filt, dtype, mode, border, box, EW.SCALE, EW.BIAS, layout)
                        assert got[j].dtype == exp.dtype and got[j].tobytes() == exp.tobytes(), \
                            (name, j, grid, dtype, layout, filt, mode, size, box, np.argwhere(got[j] != exp)[:4])
    assert k == 32


@pytest.mark.parametrize("size", SIZES)
def test_every_width_on_every_crop_and_grid(size):
    """RGB8 and grey 16, uint, every crop and grid at every output width, rows per task 2, five workgroups"""
    k = 0
    for ch, P in ((3, 8), (1, 16)):
        src = EW._source(ch, P)
        for box in BOXES:
            for grid in GRIDS:
                k += 1
                ms = matrices(box[2], box[3], size)
                qs = fields(grid, len(ms), seed=100 + k)
                filt, mode = ((WR.BILINEAR, WR.CONSTANT), (WR.NEAREST, WR.CLAMP), (WR.BILINEAR, WR.CLAMP))[k % 3]
                got = run_elastic([src], [(0, box, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, "uint", "hwc", filt, mode,
                                  (9, 8, 7, 6), run=2, grid=5)
                for j, name in enumerate(ms):
                    exp = ER.warp(src, size, ms[name], qs[j], filt, "uint", mode, (9, 8, 7, 6), box)
                    assert np.array_equal(got[j], exp), (name, j, grid, ch, P, box, filt, mode, np.argwhere(got[j] != exp)[:4])


def test_nodes_at_the_limit_under_matrices_at_their_limits():
    """nodes of +-2^28 under linear entries of +-32768 and translations of +-2^24: the sums of the position stay in int64"""
    src, box, size = EW._source(3, 8), BOXES[2], (4, 65)
    ms = EW.matrices(box[2], box[3], size)
    names = ("linear entries 32768", "linear entries -32768", "translation +2^24", "translation -2^24", "identity")
    for grid in GRIDS:
        qs = [at_the_limit(grid, s) for s in (1, -1, 1, -1, 1)]
        for filt in (WR.BILINEAR, WR.NEAREST):
            for mode in (WR.CONSTANT, WR.CLAMP):
                got = run_elastic([src], [(0, box, ms[n], qf) for n, qf in zip(names, qs)], size, grid, "uint", "hwc", filt, mode,
                                  (9, 8, 7, 6), run=1, grid=3)
                for j, n in enumerate(names):
                    exp = ER.warp(src, size, ms[n], qs[j], filt, "uint", mode, (9, 8, 7, 6), box)
                    assert np.array_equal(got[j], exp), (n, grid, filt, mode)
    Dx, _ = ER.displacement(size, at_the_limit((2, 2)))
    assert ms["linear entries 32768"][0] == 1 << 31 and int(np.abs(Dx).max()) << 31 > 1 << 58  # (m00 Dx before its shift)


# ---- no field and a field of zeros: the OUTPUT of the existing warp kernels -----------------------------------------------------------

def test_no_field_and_zeros_give_the_output_of_the_warp_kernels():
    src = EW._source(4, 8)
    lab = EW._label_sources()
    csrc = ECL._sources()["blocky"]
    box, size, grid = BOXES[2], (5, 65), (3, 5)
    ms = EW.matrices(box[2], box[3], size)
    zs = [None if k % 2 else np.zeros(grid + (2,), np.int64) for k in range(len(ms))]
    for filt, mode, dtype in ((WR.BILINEAR, WR.CONSTANT, "float32"), (WR.NEAREST, WR.CLAMP, "uint")):
        want = EW.run_warp([src], [(0, box, m) for m in ms.values()], size, dtype, "chw", filt, mode, (1, 2, 3, 4), run=2, grid=3)
        got = run_elastic([src], [(0, box, m, z) for m, z in zip(ms.values(), zs)], size, grid, dtype, "chw", filt, mode, (1, 2, 3, 4),
                          run=2, grid=3)
        assert got.tobytes() == want.tobytes(), (filt, mode)
    for sb, dtype, lut in ((1, "int64", EW.LUT), (2, "uint16", None)):
        want = EW.run_label_warp([lab[sb]], [(0, box, m) for m in ms.values()], size, dtype, WR.CONSTANT, 255, lut, run=2)
        got = run_label_elastic([lab[sb]], [(0, box, m, z) for m, z in zip(ms.values(), zs)], size, grid, dtype, WR.CONSTANT, 255, lut,
                                run=2)
        assert got.tobytes() == want.tobytes(), (sb, dtype)
    cmap = {k: i for i, k in enumerate(ECL._sources()["c7"][:5])}
    for maps in (None, [cmap]):
        dtype = "int32" if maps is None else "uint8"
        want = ECL.run_warp([csrc], [(0, box, 0, m) for m in ms.values()], size, dtype, maps, 250, WR.CONSTANT, 7, run=2)
        got = run_color_label_elastic([csrc], [(0, box, 0, m, z) for m, z in zip(ms.values(), zs)], size, grid, dtype, maps, 250,
                                      WR.CONSTANT, 7, run=2)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], maps
    srcs, mats = EC._sources(3, 8), EC._matrices()
    rot, _ = EC._warps(srcs)
    want, _ = EC.run_warp(srcs, mats, rot, EC.WARP_TO, "float16", "hwc", WR.BILINEAR, WR.CONSTANT, (9, 8, 7, 6), run=7, grid=5)
    got, _ = run_elastic_color(srcs, mats, rot, [zs[k % 2] for k in range(len(srcs))], EC.WARP_TO, grid, "float16", "hwc", WR.BILINEAR,
                               WR.CONSTANT, (9, 8, 7, 6), run=7, grid=5)
    assert got.tobytes() == want.tobytes()


# ---- the held grid ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS)
def test_one_workgroup_alternates_between_two_files_fields(grid):
    """grid = 1: ONE workgroup takes every task; the jobs are cut into tasks of one row and interleave two sources and two fields
    (A, B, A, B, ...), and a run of jobs shares one field, so the workgroup both re-stages and keeps its grid"""
    srcs = [EW._source(3, 8), EW._source(3, 8)[::-1].copy()]
    box, size = BOXES[2], (4, 65)
    m = EW.matrices(box[2], box[3], size)["30 degrees, scale 0.7"]
    A, B = smooth(grid, 1, 5.0), smooth(grid, 2, 5.0)
    seq = [A, B, A, B, B, B, None, A, None, None, A, A]
    jobs = [(k % 2, box, m, qf) for k, qf in enumerate(seq)]
    got = run_elastic(srcs, jobs, size, grid, "uint", "hwc", WR.BILINEAR, WR.CONSTANT, (9, 8, 7, 6), run=1, grid=1)
    for k, (si, _, _, qf) in enumerate(jobs):
        assert np.array_equal(got[k], ER.warp(srcs[si], size, m, qf, WR.BILINEAR, "uint", WR.CONSTANT, (9, 8, 7, 6), box)), k


# ---- the colour matrix --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch,P", EC.FORMATS)
def test_elastic_color_kernel_against_the_reference(ch, P):
    srcs, mats = EC._sources(ch, P), EC._matrices()
    size = EC.WARP_TO
    rot, _ = EC._warps(srcs)
    border = [(1 << P) - 1, (1 << P) // 4, 0, (1 << P) // 2]
    k = 0
    for layout, mode, filt, dtypes in (("hwc", WR.CONSTANT, WR.BILINEAR, EC.DTYPES), ("chw", WR.CONSTANT, WR.NEAREST, ["uint", "float32"]),
                                       ("chw", WR.CLAMP, WR.BILINEAR, ["uint", "bfloat16"]), ("hwc", WR.CLAMP, WR.NEAREST, ["float16"])):
        for dtype in dtypes:
            grid = GRIDS[k % len(GRIDS)]
            k += 1
            qs = fields(grid, len(srcs), seed=300 + k)
            got, n = run_elastic_color(srcs, mats, rot, qs, size, grid, dtype, layout, filt, mode, border, run=9, grid=5)
            for i, s in enumerate(srcs):
                want = ER.warp_mixed(s, size, rot[i], qs[i], mats[i], filt, dtype, mode, border, None, EC.SCALE, EC.BIAS, layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (ch, P, layout, filt, mode, dtype, i, np.argwhere(got[i] != want)[:4])


# ---- labels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(LR.DTYPES))
def test_label_elastic_every_dtype_source_lut_and_border(dtype):
    src = EW._label_sources()
    cases = [(1, None), (1, EW.LUT if dtype in ("int32", "int64") else EW.LUT + 100)]
    if dtype != "uint8":
        cases.append((2, None))
    k = 0
    for sb, lut in cases:
        for mode, bl in ((WR.CONSTANT, 255), (WR.CONSTANT, -1), (WR.CLAMP, 0)):
            if bl < 0 and dtype in ("uint8", "uint16"):
                continue  # (the host refuses it: BAD_ARG)
            for box in BOXES:
                size, grid = SIZES[k % len(SIZES)], GRIDS[k % len(GRIDS)]
                k += 1
                ms = matrices(box[2], box[3], size)
                qs = fields(grid, len(ms), seed=500 + k)
                got = run_label_elastic([src[sb]], [(0, box, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, dtype, mode, bl, lut,
                                        run=2, grid=k % 4)
                for j, name in enumerate(ms):
                    exp = ER.warp_labels(src[sb].astype(np.uint32), size, ms[name], qs[j], mode, bl, box, lut, dtype)
                    assert got[j].dtype == exp.dtype and np.array_equal(got[j], exp), (name, j, grid, dtype, sb, mode, bl, box, size)


def test_the_label_pick_is_the_image_nearest_pick():
    """(d) a source whose value encodes its own coordinates, as a two-channel 16-bit image, as 16-bit labels and as an RGB mask:
    under one matrix and one field the three kernels name the same source pixel, and border where the others have border"""
    h, w = 12, 17
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx, yy], axis=2).astype(np.uint16)
    lab = (yy * 256 + xx).astype(np.uint16)
    rgb = np.stack([xx, yy, np.zeros_like(xx)], axis=2).astype(np.uint8)
    box = BOXES[2]
    for size, grid in (((7, 13), (3, 5)), ((9, 65), (33, 33))):
        ms = matrices(box[2], box[3], size)
        qs = [smooth(grid, 700 + k, 2.5) for k in range(len(ms))]
        for mode in (WR.CONSTANT, WR.CLAMP):
            pix = run_elastic([img], [(0, box, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, "uint", "hwc", WR.NEAREST, mode,
                              (0xFFFF, 0xFFFF, 0, 0), run=4)
            lbl = run_label_elastic([lab], [(0, box, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, "int32", mode, -1, run=4)
            clb, _ = run_color_label_elastic([rgb], [(0, box, 0, m, qf) for m, qf in zip(ms.values(), qs)], size, grid, "int32", None, -1,
                                             mode, -1, run=4)
            for j, name in enumerate(ms):
                assert np.array_equal(lbl[j], clb[j]), name  # (R | G << 8 is y * 256 + x as well)
                out_of_crop = lbl[j] == -1
                assert np.array_equal(out_of_crop, pix[j][:, :, 0] == 0xFFFF), name
                assert mode == WR.CONSTANT or not out_of_crop.any()
                inside = ~out_of_crop
                assert np.array_equal(lbl[j][inside], (pix[j][:, :, 1].astype(np.int32) * 256 + pix[j][:, :, 0])[inside]), name


# ---- colour labels --------------------------------------------------------------------------------------------------------------------

def _check_color_labels(srcs, jobs, size, nodes, dtype, maps=None, missing=-1, mode=WR.CONSTANT, border_label=0, **kw):
    got, um = run_color_label_elastic(srcs, jobs, size, nodes, dtype, maps, missing, mode, border_label, **kw)
    for k, (si, box, mi, m, qf) in enumerate(jobs):
        exp, miss = ER.warp_color_labels(srcs[si], size, m, qf, mode, border_label, box, None if maps is None else maps[mi], missing, dtype)
        assert got[k].dtype == exp.dtype and got[k].tobytes() == exp.tobytes(), (dtype, size, nodes, box, mi, m, np.argwhere(got[k] != exp)[:4])
        assert um[k] == miss, (dtype, size, box, mi, m, um[k], miss)
    return um


@pytest.mark.parametrize("mode", [WR.CONSTANT, WR.CLAMP])
def test_color_label_elastic_pack_and_map(mode):
    S = ECL._sources()
    srcs = [S["blocky"], S["noisy"]]
    few = {k: i + 1 for i, k in enumerate(S["c7"][:5])}  # two of the seven colours are missing
    many = {k: i % 250 for i, k in enumerate(S["c2300"][:2048])}
    k, misses = 0, 0
    for size in ((3, 1), (5, 7), (6, 64), (4, 65), (3, 257)):
        for box in ECL.BOXES[1:4]:
            bw, bh = box[2], box[3]
            ms = list(matrices(bw, bh, size).values())
            grid = GRIDS[k % len(GRIDS)]
            k += 1
            qs = fields(grid, len(ms), seed=900 + k)
            # tasks of two images, hence two tables and two fields, alternate in one workgroup (grid 2 or 3); border_label == missing
            jobs = [(j % 2, box, j % 2, m, qs[j]) for j, m in enumerate(ms)]
            for dtype in (("uint8", "int64") if k % 2 else ("uint16", "int32")):
                misses += sum(_check_color_labels(srcs, jobs, size, grid, dtype, [few, many], 251, mode, 251, run=2, grid=2 + k % 2))
            _check_color_labels(srcs, jobs, size, grid, "int32" if k % 2 else "int64", None, -1, mode, -5, run=2, grid=k % 3)
    assert misses > 0


# ---- tasks that break a bound (the emulator only) -------------------------------------------------------------------------------------

def _elastic(task, off, gw, gh):
    T = EL.elastic_task_type(type(task))
    return T(w=task, field_off=off, grid_w=gw, grid_h=gh)


def test_tasks_that_break_a_bound_are_skipped():
    """every bound of the warp twin, a grid dimension outside 2 .. 33, a misaligned field_off, and a node above 2^28 in magnitude
    anywhere in the grid -- also after a good task of the same workgroup, and with the bad field named twice in a row"""
    H, W = 6, 20
    ident = [65536, 0, 0, 0, 65536, 0]
    good_q = smooth((3, 5), 11)
    bad_first, bad_last, bad_neg = good_q.copy(), good_q.copy(), good_q.copy()
    bad_first[0, 0, 0] = LIMIT + 1
    bad_last[2, 4, 1] = LIMIT + 1
    bad_neg[1, 2, 0] = -LIMIT - 1
    big = np.zeros((33, 33, 2), np.int64)
    big[32, 32, 1] = -LIMIT - 1  # the last node a workgroup stages
    fbuf, (o_good, o_first, o_last, o_neg, o_big) = EL.fields_buffer([good_q, bad_first, bad_last, bad_neg, big])
    good = (o_good, 5, 3)
    ela_bad = [(o_good, 1, 3), (o_good, 5, 1), (o_good, 0, 0), (o_good, 34, 3), (o_good, 5, 34), (o_good, 65535, 3), (o_good + 4, 5, 3),
               (o_good + 1, 5, 3), (o_first, 5, 3), (o_last, 5, 3), (o_neg, 5, 3), (o_neg, 5, 3), (o_big, 33, 33),
               (EL.NO_FIELD, 1, 3), (EL.NO_FIELD, 5, 34)]
    L = EL._emu()

    # the image kernel (and the colour kernel: the same predicate in front of the record's)
    a, soff = EW._arena([EW._source(3, 8), EW._source(1, 16)])
    base = dict(src_off=soff[0], out_off=0, src_pitch=17 * 3, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, out_sx=3,
                out_sy=3 * W, out_sc=1, channels=3, bits=8, dtype=1, filter=0, border_mode=0)
    warp_bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
                dict(crop_h=0), dict(crop_w=1 << 31), dict(channels=0), dict(channels=5), dict(bits=12), dict(dtype=4), dict(filter=1),
                dict(filter=3), dict(border_mode=2), dict(bits=16, channels=1, src_off=soff[1] + 1)]

    def image_task(e, m=ident, **kw):
        t = EW.WarpTask(**dict(base, **kw))
        t.m[:] = m
        return _elastic(t, *e)

    tasks = [image_task(good, **b) for b in warp_bad] + [image_task(e) for e in ela_bad]
    tasks += [image_task(good, m=[(1 << 31) + 1, 0, 0, 0, 65536, 0]), image_task(good, m=[65536, 0, 0, 0, 65536, -(1 << 40) - 1])]
    n = len(tasks)
    out = EW._aligned(4096 + H * W * 3 * 4 + 4096, FILL)
    for g in (0, 1):  # one workgroup per task; one workgroup for all, which stages and votes task after task
        assert L.emu_png_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), fbuf.ctypes.data, n, g) == 0
        assert (out == FILL).all()
    # a good task, then bad ones, then the good one again, in ONE workgroup: the held verdicts do not leak
    ok = image_task(good, dtype=0)
    seq = [ok, image_task((o_last, 5, 3)), image_task((o_last, 5, 3)), image_task((o_good, 5, 34))]
    assert L.emu_png_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 4)(*seq), fbuf.ctypes.data, 4, 1) == 0
    want = ER.warp(EW._source(3, 8), (H, W), ident, good_q, WR.BILINEAR)
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), want)
    out[:] = FILL
    seq = [image_task((o_neg, 5, 3)), ok]
    assert L.emu_png_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 2)(*seq), fbuf.ctypes.data, 2, 1) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), want)

    rec = np.frombuffer(EC._records([np.eye(3, 4)], 8), np.uint8).copy()
    cbase = dict(base, color_off=0)

    def color_task(e, **kw):
        t = EC.WarpColorTask(**dict(cbase, **kw))
        t.m[:] = ident
        return _elastic(t, *e)

    tasks = [color_task(good, **b) for b in warp_bad + [dict(channels=1), dict(channels=2), dict(color_off=4)]] + [color_task(e) for e in ela_bad]
    n = len(tasks)
    out[:] = FILL
    assert L.emu_png_elastic_color_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), rec.ctypes.data,
                                         fbuf.ctypes.data, n, 0) == 0
    assert (out == FILL).all()
    ok = color_task(good, dtype=0)
    assert L.emu_png_elastic_color_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), rec.ctypes.data, fbuf.ctypes.data, 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), want)

    # the label kernel
    lab = EW._label_sources()
    a, soff = EW._arena([lab[1], lab[2]])
    lbase = dict(src_off=soff[0], out_off=0, src_pitch=17, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, border_label=3,
                 src_bytes=1, dtype=3, border_mode=0)
    label_bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
                 dict(crop_h=0), dict(crop_h=1 << 31), dict(src_bytes=0), dict(src_bytes=3), dict(dtype=4),
                 dict(dtype=0, src_bytes=2, src_off=soff[1]), dict(border_mode=2), dict(src_bytes=2, src_off=soff[1] + 1)]

    def label_task(e, m=ident, **kw):
        t = EW.LabelWarpTask(**dict(lbase, **kw))
        t.m[:] = m
        return _elastic(t, *e)

    tasks = [label_task(good, **b) for b in label_bad] + [label_task(e) for e in ela_bad] + [label_task(good, m=[1 << 32, 0, 0, 0, 65536, 0])]
    n = len(tasks)
    out = EW._aligned(4096 + H * W * 8 + 4096, FILL)
    for g in (0, 1):
        assert L.emu_png_label_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), None, fbuf.ctypes.data,
                                             n, g) == 0
        assert (out == FILL).all()
    ok = label_task(good)
    assert L.emu_png_label_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), None, fbuf.ctypes.data, 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W),
                          ER.warp_labels(lab[1], (H, W), ident, good_q, WR.CONSTANT, 3))

    # the colour-label kernel
    rgb = ECL._sources()["blocky"]
    a = np.frombuffer(bytes(16) + rgb.tobytes(), np.uint8).copy()
    cl = dict(src_off=16, out_off=0, src_pitch=37, crop_w=37, crop_h=29, out_w=W, out_h=H, row0=0, rows=H, border_label=3, image=0,
              dtype=3, mode=0, border_mode=0)
    clbl_bad = [dict(out_w=0), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(crop_w=0), dict(crop_h=1 << 31), dict(dtype=4),
                dict(mode=2), dict(border_mode=2), dict(dtype=1), dict(mode=1, map_slots=3), dict(mode=1, map_slots=8, map_off=8)]

    def clbl_task(e, **kw):
        return _elastic(ECL._task(ident, **dict(cl, **kw)), *e)

    tasks = [clbl_task(good, **b) for b in clbl_bad] + [clbl_task(e) for e in ela_bad]
    n = len(tasks)
    out[:] = FILL
    cnt = np.zeros(1, np.uint32)
    tb = EW._aligned(64, 0)
    for g in (0, 1):
        assert L.emu_png_color_label_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), tb.ctypes.data,
                                                   cnt.ctypes.data, fbuf.ctypes.data, n, g) == 0
        assert (out == FILL).all() and cnt[0] == 0
    ok = clbl_task(good)
    assert L.emu_png_color_label_elastic_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), tb.ctypes.data, None,
                                               fbuf.ctypes.data, 1, 0) == 0
    exp, _ = ER.warp_color_labels(rgb, (H, W), ident, good_q, WR.CONSTANT, 3, None, None, -1, "int64")
    assert np.array_equal(out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W), exp)
