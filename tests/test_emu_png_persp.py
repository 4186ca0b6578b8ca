"""The four kernels of the perspective warp (csrc/png_persp_kernel.inc) on the CPU lock-step emulator, BIT FOR BIT against the
numpy restatement tests/png_persp_ref.py.  The runners, sources, crops, output sizes, arenas and sentinels are those of the warp
batteries (test_emu_png_warp, test_emu_png_color, test_emu_png_color_labels_warp): tests/map_launch.py extends their tasks by p[]
and launches the persp twin, so the shapes are the smallest at which these kernels go wrong --
  * crops of 1 x 1, 1 x 9 and 13 x 7 inside a larger image at odd arena offsets; output widths 1, 7, 64, 65 and 257; task runs that
    do not divide out_h; fewer workgroups than tasks; channels 1 - 4, P = 8 / 16, all dtypes, both layouts, filters and borders;
  * labels of 1 and 2 bytes with and without a LUT; colour labels in PACK and MAP with `unmatched` compared; the colour matrix.
The matrices (matrices() below): random keystones; the affine set with row 2 = (0, 0, 1), also asserted equal to the OUTPUT of the
existing warp kernels; x 2 and x 1/2 of a whole matrix; D at 2^21 at one corner and at 2^33 - 1 at the opposite one; numerators
near 2^48 over D = 2^21 (|U| about 2^58: border under CONSTANT, an edge pixel under CLAMP); maps that leave the crop on the
negative side.  Tasks that break a bound are skipped with the sentinels intact (emulator only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_launch as PL  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_persp_ref as PR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_emu_png_color as EC  # noqa: E402
import test_emu_png_color_labels_warp as ECL  # noqa: E402
import test_emu_png_warp as EW  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from debigulator_amd.api import png_perspective_matrix  # noqa: E402

ONE = 1 << 30  # 1.0 in row 2
FILL = EW.FILL
BOXES, SIZES = EW.BOXES, EW.SIZES


# ---- the matrices --------------------------------------------------------------------------------------------------------------

def q(M):
    m = PR.quantise(np.asarray(M, dtype=np.float64).reshape(-1))
    assert m is not None, M
    return m


def keystone(cw, chh, size, rng):
    """a random quadrilateral of the crop (its corners moved by up to 0.35 of the crop, also outside it) onto the output -> (the
    3 x 3 matrix in float64, its nine integers); on an output of one pixel on an axis row 2 grows as the quadrilateral does, so the
    move shrinks until the map is inside the limits"""
    move = rng.uniform(-0.35, 0.35, (4, 2)) * (cw, chh)
    for shrink in (1.0, 0.5, 0.2, 0.05, 0.01):
        M = png_perspective_matrix(np.array([(0, 0), (cw, 0), (cw, chh), (0, chh)]) + shrink * move, size)
        m = PR.quantise([v for r in M for v in r])
        if m is not None and PR.range_ok(m, size) and (m[6] or m[7]):
            return M, m
    raise AssertionError((cw, chh, size))


def keystones(cw, chh, size, n=3, seed=0):
    rng = np.random.default_rng(1000 * cw + 10 * chh + size[1] + seed)
    return {"keystone %d" % k: keystone(cw, chh, size, rng)[1] for k in range(n)}


def d_at_corners(size):
    """{name: p[]} with D growing along x (along y on a one-pixel-wide output): D == 2^21 at pixel (0, 0) and as near below 2^33 at
    the last pixel as the steps allow; D == 2^33 - 1 at the last pixel and as near above 2^21 at pixel (0, 0).  (D has the parity of
    p0 + p1 at every pixel, so the two limits never meet in one matrix.)  On a 1 x 1 output: each limit by itself."""
    H, W = size
    steps = W - 1 if W > 1 else H - 1
    if steps == 0:
        return {"D = 2^21": (0, 0, PR.D_MIN // 2), "D = 2^33 - 1": (1, 0, PR.D_MAX // 2)}
    slope = (PR.D_MAX - PR.D_MIN) // (2 * steps)
    even, odd = slope & ~1, slope - 1 + (slope & 1)
    d0 = PR.D_MAX - 2 * odd * steps
    rows = {"D from 2^21": (even, (PR.D_MIN - even) // 2), "D up to 2^33 - 1": (odd, (d0 - odd) // 2)}
    return {k: (a, 0, c) if W > 1 else (0, a, c) for k, (a, c) in rows.items()}


def matrices(cw, chh, size):
    """name -> the nine quantised integers; every one is in range on `size`"""
    H, W = size
    ms = keystones(cw, chh, size)
    k0 = [v // 4 * 2 for v in ms["keystone 0"]]  # about half of it (x 2 stays in range), every entry even (x 1/2 is exact)
    ms["keystone 0, even"] = k0
    ms["keystone 0 x 2"] = [2 * v for v in k0]
    ms["keystone 0 x 1/2"] = [v // 2 for v in k0]
    for name, p in d_at_corners(size).items():
        ms[name] = [4 * 65536 * cw // W, 0, 0, 0, 4 * 65536 * chh // H, 0] + list(p)  # (inside the crop where D is above 2^31)
    aff = EW.matrices(cw, chh, size)
    ms["far, positive"] = aff["translation +2^24"][:6] + [0, 0, PR.D_MIN // 2]  # D = 2^21: the affine position times 1024
    ms["far, negative"] = aff["translation -2^24"][:6] + [0, 0, PR.D_MIN // 2]
    ms["negative side"] = q([[1.25, 0.1, -0.75 * cw - 0.3], [0.05, 0.9, -0.6 * chh - 0.2], [0.002, 0.001, 1.0]])
    for name, m in ms.items():
        assert PR.range_ok(m, size), (name, size)
    return ms


def affine_as_persp(cw, chh, size):
    return {k: list(m) + [0, 0, ONE] for k, m in EW.matrices(cw, chh, size).items()}


def test_the_special_matrices_hit_what_they_are_for():
    size = (5, 257)
    ms = matrices(13, 7, size)
    for name in ("D from 2^21", "D up to 2^33 - 1"):
        _, _, D = PR.parts(size, ms[name])
        assert (int(D[0, 0]) == PR.D_MIN) if name == "D from 2^21" else (int(D[-1, -1]) == PR.D_MAX), name
        assert int(D.min()) == int(D[0, 0]) < 1 << 22 and int(D.max()) == int(D[-1, -1]) > (1 << 33) - 2048, name
    assert [int(PR.parts((1, 1), [0] * 6 + list(p))[2][0, 0]) for p in d_at_corners((1, 1)).values()] == [PR.D_MIN, PR.D_MAX]
    for name, sign in (("far, positive", 1), ("far, negative", -1)):
        U, V = PR.positions(size, ms[name])
        assert int((sign * U).min()) > 1 << 50 and int((sign * V).min()) > 1 << 50, name
    for m in NEAR_2_48:
        for X in (16383, 16000):
            n = [abs(v) for v in _last_row_numerators(m, X)]
            assert 1 << 47 < min(n) and max(n) < 1 << 48 and min(n) << 10 > 1 << 57
    # floor, not truncation: negative numerators that leave a remainder
    NU, NV, D = PR.parts(size, ms["negative side"])
    assert ((NU < 0) & (NU % D != 0)).any() and ((NV < 0) & (NV % D != 0)).any()
    U, _ = PR.positions(size, ms["negative side"])
    assert (U >> 17).min() < 0 and ((U >> 17) >= 0).any()  # leaves the crop on the negative side, not everywhere
    # x 2 and x 1/2 change no position; row 2 = (0, 0, 1) is the affine rule
    for a in ("keystone 0 x 2", "keystone 0 x 1/2"):
        assert all(np.array_equal(x, y) for x, y in zip(PR.positions(size, ms[a]), PR.positions(size, ms["keystone 0, even"]))), a
    for name, m in affine_as_persp(13, 7, size).items():
        assert all(np.array_equal(x, y) for x, y in zip(PR.positions(size, m), WR.positions(size, m[:6]))), name
    # the keystones are no affine maps, and their picks land inside the crop somewhere
    for k in range(3):
        m = ms["keystone %d" % k]
        jx, jy = PR.picks(size, m)
        assert (m[6] or m[7]) and ((jx >= 0) & (jx < 13) & (jy >= 0) & (jy < 7)).any()


# ---- the runners of the warp batteries, through the persp kernels -----------------------------------------------------------------

def run_persp(srcs, jobs, size, *a, **kw):
    """jobs: [(source index, box, m9)] -> EW.run_warp's result from debig_png_persp_kernel"""
    with PL.as_persp(EW, [m[6:] for _, _, m in jobs]):
        return EW.run_warp(srcs, [(si, box, m[:6]) for si, box, m in jobs], size, *a, **kw)


def run_label_persp(srcs, jobs, size, *a, **kw):
    with PL.as_persp(EW, [m[6:] for _, _, m in jobs]):
        return EW.run_label_warp(srcs, [(si, box, m[:6]) for si, box, m in jobs], size, *a, **kw)


def run_color_label_persp(srcs, jobs, size, *a, **kw):
    """jobs: [(source index, box, map index, m9)]"""
    with PL.as_persp(ECL, [j[3][6:] for j in jobs]):
        return ECL.run_warp(srcs, [(si, box, mi, m[:6]) for si, box, mi, m in jobs], size, *a, **kw)


def run_persp_color(srcs, mats, ms, size, *a, **kw):
    with PL.as_persp(EC, [m[6:] for m in ms]):
        return EC.run_warp(srcs, mats, [m[:6] for m in ms], size, *a, **kw)


# ---- the image kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_persp_format_grid(ch, P):
    """every dtype x layout x filter x border mode, each on every matrix; crops and sizes rotate as in the warp battery"""
    src = EW._source(ch, P)
    border = [(1 << P) - 1, 0, 77, 1 << (P - 1)]
    k = 0
    for dtype in Z.DTYPES:
        for layout in ("hwc", "chw"):
            for filt in (WR.BILINEAR, WR.NEAREST):
                for mode in (WR.CONSTANT, WR.CLAMP):
                    size, box = SIZES[(k + k // 5) % len(SIZES)], BOXES[k % len(BOXES)]
                    k += 1
                    ms = matrices(box[2], box[3], size)
                    got = run_persp([src], [(0, box, m) for m in ms.values()], size, dtype, layout, filt, mode, border,
                                    run=3 if size[0] > 3 else None, grid=0 if k % 3 else 4)
                    for j, name in enumerate(ms):
                        exp = PR.warp(src, size, ms[name], filt, dtype, mode, border, box, EW.SCALE, EW.BIAS, layout)
                        assert got[j].dtype == exp.dtype and got[j].tobytes() == exp.tobytes(), \
                            (name, dtype, layout, filt, mode, size, box, np.argwhere(got[j] != exp)[:4])
    assert k == 32


@pytest.mark.parametrize("size", SIZES)
def test_every_width_on_every_crop(size):
    """RGB8 and grey 16, uint, every crop and every matrix at every output width, rows per task 2, five workgroups"""
    for ch, P in ((3, 8), (1, 16)):
        src = EW._source(ch, P)
        for box in BOXES:
            ms = matrices(box[2], box[3], size)
            for filt, mode in ((WR.BILINEAR, WR.CONSTANT), (WR.NEAREST, WR.CLAMP), (WR.BILINEAR, WR.CLAMP)):
                got = run_persp([src], [(0, box, m) for m in ms.values()], size, "uint", "hwc", filt, mode, (9, 8, 7, 6), run=2, grid=5)
                for j, name in enumerate(ms):
                    exp = PR.warp(src, size, ms[name], filt, "uint", mode, (9, 8, 7, 6), box)
                    assert np.array_equal(got[j], exp), (name, ch, P, box, filt, mode, np.argwhere(got[j] != exp)[:4])


def test_far_positions_are_border_or_an_edge_pixel():
    """|U| about 2^51: every element is the border under CONSTANT and one pixel of the crop's edge under CLAMP"""
    src, box, size = EW._source(3, 8), BOXES[2], (4, 65)
    crop = src[box[1]: box[1] + box[3], box[0]: box[0] + box[2]]
    ms = matrices(box[2], box[3], size)
    for name in ("far, positive", "far, negative"):
        for filt in (WR.BILINEAR, WR.NEAREST):
            got = run_persp([src], [(0, box, ms[name])], size, "uint", "hwc", filt, WR.CONSTANT, (9, 8, 7, 6))[0]
            jx, jy = PR.picks(size, ms[name])
            far = (np.abs(jx) > 1 << 30) | (np.abs(jy) > 1 << 30)
            assert far.sum() > far.size // 2 and (got[far] == (9, 8, 7)).all(), (name, filt)
            got = run_persp([src], [(0, box, ms[name])], size, "uint", "hwc", filt, WR.CLAMP)[0]
            edge = crop[np.clip(jy, 0, box[3] - 1), np.clip(jx, 0, box[2] - 1)]
            assert np.array_equal(got[far], edge[far]), (name, filt)


# numerators near 2^48 need cx and cy near 2^15: the LAST ROW of a 16384 x 16384 output as one task of one row whose out_sy is 0, so
# that the row lands at the start of a buffer of one row.  Rows 0 and 1 at their limits, D = 2^21 everywhere.
NEAR_2_48 = [[1 << 31, 1 << 31, 1 << 40, -(1 << 31), -(1 << 31), -(1 << 40)], [-(1 << 31), -(1 << 31), -(1 << 40), 1 << 31, 1 << 31, 1 << 40]]


def _last_row_numerators(m, X):
    cx, cy = 2 * X + 1, 2 * 16383 + 1
    return m[0] * cx + m[1] * cy + 2 * m[2], m[3] * cx + m[4] * cy + 2 * m[5]


@pytest.mark.parametrize("mode", [WR.CONSTANT, WR.CLAMP])
def test_numerators_near_2_48_over_the_smallest_denominator(mode):
    """|U|, |V| about 2^58 on every pixel: the border under CONSTANT, the crop's corner pixel of that side under CLAMP"""
    src = EW._source(1, 8)
    a, soff = EW._arena([src])
    x, y, bw, bh = BOXES[2]
    N = 16384
    for m in NEAR_2_48:
        for filt in (WR.BILINEAR, WR.NEAREST):
            t = EW.WarpTask(src_off=soff[0] + y * 17 + x, out_off=0, src_pitch=17, crop_w=bw, crop_h=bh, out_w=N, out_h=N, row0=N - 1, rows=1,
                            out_sx=1, out_sy=0, out_sc=1, channels=1, bits=8, dtype=0, filter=filt, border_mode=mode)
            t.m[:] = m
            t.border[:] = [201, 0, 0, 0]
            T = PL.persp_task_type(EW.WarpTask)
            pt = T(w=t)
            pt.p[:] = [0, 0, PR.D_MIN // 2]
            assert PR.range_ok(m + [0, 0, PR.D_MIN // 2], (N, N))
            out = EW._aligned(4096 + N + 4096, FILL)
            assert PL.launch("png_persp", a, out[4096:], (T * 1)(pt), 1, 0) == 0
            assert (out[:4096] == FILL).all() and (out[4096 + N:] == FILL).all()
            nu, nv = _last_row_numerators(m, 0)
            edge = src[y + (bh - 1 if nv > 0 else 0), x + (bw - 1 if nu > 0 else 0), 0]
            assert (out[4096: 4096 + N] == (201 if mode == WR.CONSTANT else edge)).all(), (m, filt, mode)


# ---- row 2 = (0, 0, 1): the OUTPUT of the existing warp kernels -------------------------------------------------------------------

def test_affine_matrices_give_the_output_of_the_warp_kernels():
    src = EW._source(4, 8)
    lab = EW._label_sources()
    csrc = ECL._sources()["blocky"]
    box, size = BOXES[2], (5, 65)
    ms = affine_as_persp(box[2], box[3], size)
    for filt, mode, dtype in ((WR.BILINEAR, WR.CONSTANT, "float32"), (WR.NEAREST, WR.CLAMP, "uint")):
        want = EW.run_warp([src], [(0, box, m[:6]) for m in ms.values()], size, dtype, "chw", filt, mode, (1, 2, 3, 4), run=2, grid=3)
        got = run_persp([src], [(0, box, m) for m in ms.values()], size, dtype, "chw", filt, mode, (1, 2, 3, 4), run=2, grid=3)
        assert got.tobytes() == want.tobytes(), (filt, mode)
    for sb, dtype, lut in ((1, "int64", EW.LUT), (2, "uint16", None)):
        want = EW.run_label_warp([lab[sb]], [(0, box, m[:6]) for m in ms.values()], size, dtype, WR.CONSTANT, 255, lut, run=2)
        got = run_label_persp([lab[sb]], [(0, box, m) for m in ms.values()], size, dtype, WR.CONSTANT, 255, lut, run=2)
        assert got.tobytes() == want.tobytes(), (sb, dtype)
    cmap = {k: i for i, k in enumerate(ECL._sources()["c7"][:5])}
    for maps in (None, [cmap]):
        dtype = "int32" if maps is None else "uint8"
        want = ECL.run_warp([csrc], [(0, box, 0, m[:6]) for m in ms.values()], size, dtype, maps, 250, WR.CONSTANT, 7, run=2)
        got = run_color_label_persp([csrc], [(0, box, 0, m) for m in ms.values()], size, dtype, maps, 250, WR.CONSTANT, 7, run=2)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], maps
    srcs, mats = EC._sources(3, 8), EC._matrices()
    rot, _ = EC._warps(srcs)
    want, _ = EC.run_warp(srcs, mats, rot, EC.WARP_TO, "float16", "hwc", WR.BILINEAR, WR.CONSTANT, (9, 8, 7, 6), run=7, grid=5)
    got, _ = run_persp_color(srcs, mats, [list(m) + [0, 0, ONE] for m in rot], EC.WARP_TO, "float16", "hwc", WR.BILINEAR, WR.CONSTANT,
                             (9, 8, 7, 6), run=7, grid=5)
    assert got.tobytes() == want.tobytes()


# ---- the colour matrix --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch,P", EC.FORMATS)
def test_persp_color_kernel_against_the_reference(ch, P):
    srcs, mats = EC._sources(ch, P), EC._matrices()
    size = EC.WARP_TO
    ms = [list(matrices(s.shape[1], s.shape[0], size).values())[i] for i, s in enumerate(srcs)]  # three keystones
    border = [(1 << P) - 1, (1 << P) // 4, 0, (1 << P) // 2]
    for layout, mode, filt, dtypes in (("hwc", WR.CONSTANT, WR.BILINEAR, EC.DTYPES), ("chw", WR.CONSTANT, WR.NEAREST, ["uint", "float32"]),
                                       ("chw", WR.CLAMP, WR.BILINEAR, ["uint", "bfloat16"]), ("hwc", WR.CLAMP, WR.NEAREST, ["float16"])):
        for dtype in dtypes:
            got, n = run_persp_color(srcs, mats, ms, size, dtype, layout, filt, mode, border, run=9, grid=5)
            assert n == 24
            for i, s in enumerate(srcs):
                want = PR.warp_mixed(s, size, ms[i], mats[i], filt, dtype, mode, border, None, EC.SCALE, EC.BIAS, layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (ch, P, layout, filt, mode, dtype, i, np.argwhere(got[i] != want)[:4])


# ---- labels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", list(LR.DTYPES))
def test_label_persp_every_dtype_source_lut_and_border(dtype):
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
                size = SIZES[k % len(SIZES)]
                k += 1
                ms = matrices(box[2], box[3], size)
                got = run_label_persp([src[sb]], [(0, box, m) for m in ms.values()], size, dtype, mode, bl, lut, run=2, grid=k % 4)
                for j, name in enumerate(ms):
                    exp = PR.warp_labels(src[sb].astype(np.uint32), size, ms[name], mode, bl, box, lut, dtype)
                    assert got[j].dtype == exp.dtype and np.array_equal(got[j], exp), (name, dtype, sb, mode, bl, box, size)


def test_the_label_pick_is_the_image_nearest_pick():
    """a source whose value encodes its own coordinates, as a two-channel 16-bit image, as 16-bit labels and as an RGB mask: under
    one matrix the three kernels name the same source pixel, and border where the others have border"""
    h, w = 12, 17
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([xx, yy], axis=2).astype(np.uint16)
    lab = (yy * 256 + xx).astype(np.uint16)
    rgb = np.stack([xx, yy, np.zeros_like(xx)], axis=2).astype(np.uint8)
    box = BOXES[2]
    for size in ((7, 13), (9, 65)):
        ms = matrices(box[2], box[3], size)
        for mode in (WR.CONSTANT, WR.CLAMP):
            pix = run_persp([img], [(0, box, m) for m in ms.values()], size, "uint", "hwc", WR.NEAREST, mode, (0xFFFF, 0xFFFF, 0, 0), run=4)
            lbl = run_label_persp([lab], [(0, box, m) for m in ms.values()], size, "int32", mode, -1, run=4)
            clb, _ = run_color_label_persp([rgb], [(0, box, 0, m) for m in ms.values()], size, "int32", None, -1, mode, -1, run=4)
            for j, name in enumerate(ms):
                assert np.array_equal(lbl[j], clb[j]), name  # (R | G << 8 is y * 256 + x as well)
                out_of_crop = lbl[j] == -1
                assert np.array_equal(out_of_crop, pix[j][:, :, 0] == 0xFFFF), name
                assert mode == WR.CONSTANT or not out_of_crop.any()
                inside = ~out_of_crop
                assert np.array_equal(lbl[j][inside], (pix[j][:, :, 1].astype(np.int32) * 256 + pix[j][:, :, 0])[inside]), name


# ---- colour labels --------------------------------------------------------------------------------------------------------------------

def _check_color_labels(srcs, jobs, size, dtype, maps=None, missing=-1, mode=WR.CONSTANT, border_label=0, **kw):
    got, um = run_color_label_persp(srcs, jobs, size, dtype, maps, missing, mode, border_label, **kw)
    for k, (si, box, mi, m) in enumerate(jobs):
        exp, miss = PR.warp_color_labels(srcs[si], size, m, mode, border_label, box, None if maps is None else maps[mi], missing, dtype)
        assert got[k].dtype == exp.dtype and got[k].tobytes() == exp.tobytes(), (dtype, size, box, mi, m, np.argwhere(got[k] != exp)[:4])
        assert um[k] == miss, (dtype, size, box, mi, m, um[k], miss)
    return um


@pytest.mark.parametrize("mode", [WR.CONSTANT, WR.CLAMP])
def test_color_label_persp_pack_and_map(mode):
    S = ECL._sources()
    srcs = [S["blocky"], S["noisy"]]
    few = {k: i + 1 for i, k in enumerate(S["c7"][:5])}  # two of the seven colours are missing
    many = {k: i % 250 for i, k in enumerate(S["c2300"][:2048])}
    k, misses = 0, 0
    for size in ((3, 1), (5, 7), (6, 64), (4, 65), (3, 257)):
        for box in ECL.BOXES[1:4]:
            bw, bh = box[2], box[3]
            ms = list(matrices(bw, bh, size).values())
            k += 1
            # tasks of two images, hence two tables, alternate in one workgroup (grid 2 or 3); border_label == missing
            jobs = [(j % 2, box, j % 2, m) for j, m in enumerate(ms)]
            for dtype in (("uint8", "int64") if k % 2 else ("uint16", "int32")):
                misses += sum(_check_color_labels(srcs, jobs, size, dtype, [few, many], 251, mode, 251, run=2, grid=2 + k % 2))
            _check_color_labels(srcs, jobs, size, "int32" if k % 2 else "int64", None, -1, mode, -5, run=2, grid=k % 3)
    assert misses > 0


# ---- tasks that break a bound (the emulator only) -------------------------------------------------------------------------------------

def _persp(task, p):
    T = PL.persp_task_type(type(task))
    t = T(w=task)
    t.p[:] = p
    return t


def test_tasks_that_break_a_bound_are_skipped():
    """every bound of the warp twin, |p_k| above 2^32, and D out of range at each corner -- also where only a pixel OUTSIDE the
    task's own rows breaks it, and where the one row of the task is the bad one"""
    H, W = 6, 20
    ident = [65536, 0, 0, 0, 65536, 0]
    good = [0, 0, ONE]
    far_x, far_y = 2 * W - 1, 2 * H - 1
    bad_p = [[(1 << 32) + 1, 0, -(1 << 32)], [0, -(1 << 32) - 1, 1 << 32], [0, 0, (1 << 32) + 1], [0, 0, 0], [0, 0, -ONE],
             [0, 0, PR.D_MIN // 2 - 1], [1, 0, PR.D_MIN // 2 - 1], [1, 0, PR.D_MAX // 2 + 2 - W],  # D just below / just above at a corner
             [-(1 << 26), 0, ONE],   # D falls below 2^21 towards the right-hand corners only
             [0, -(1 << 28), ONE],   # ... towards the bottom corners only (the first rows alone would pass)
             [1 << 27, 1 << 29, ONE]]  # above 2^33 - 1 at the last pixel only
    for p in bad_p:
        assert not PR.range_ok(ident + p, (H, W)), p
    for p in ([0, 0, PR.D_MIN // 2], [1, 0, PR.D_MAX // 2 + 1 - W], good):  # (the limits themselves are inside)
        assert PR.range_ok(ident + p, (H, W)), p
    L = PL._emu()

    # the image kernel (and the colour kernel: the same predicate in front of the record's)
    a, soff = EW._arena([EW._source(3, 8), EW._source(1, 16)])
    base = dict(src_off=soff[0], out_off=0, src_pitch=17 * 3, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, out_sx=3,
                out_sy=3 * W, out_sc=1, channels=3, bits=8, dtype=1, filter=0, border_mode=0)
    warp_bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
                dict(crop_h=0), dict(crop_w=1 << 31), dict(channels=0), dict(channels=5), dict(bits=12), dict(dtype=4), dict(filter=1),
                dict(filter=3), dict(border_mode=2), dict(bits=16, channels=1, src_off=soff[1] + 1)]

    def image_task(p, m=ident, **kw):
        t = EW.WarpTask(**dict(base, **kw))
        t.m[:] = m
        return _persp(t, p)

    tasks = [image_task(good, **b) for b in warp_bad] + [image_task(p) for p in bad_p] + [image_task(p, row0=0, rows=1) for p in bad_p]
    tasks += [image_task(good, m=[(1 << 31) + 1, 0, 0, 0, 65536, 0]), image_task(good, m=[65536, 0, 0, 0, 65536, -(1 << 40) - 1])]
    n = len(tasks)
    out = EW._aligned(4096 + H * W * 3 * 4 + 4096, FILL)
    assert L.emu_png_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), n, 0) == 0
    assert (out == FILL).all()
    ok = image_task(good, dtype=0)
    assert L.emu_png_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), WR.warp(EW._source(3, 8), (H, W), ident, WR.BILINEAR))

    rec = np.frombuffer(EC._records([np.eye(3, 4)], 8), np.uint8).copy()
    cbase = dict(base, color_off=0)

    def color_task(p, **kw):
        t = EC.WarpColorTask(**dict(cbase, **kw))
        t.m[:] = ident
        return _persp(t, p)

    tasks = [color_task(good, **b) for b in warp_bad + [dict(channels=1), dict(channels=2), dict(color_off=4)]] + [color_task(p) for p in bad_p]
    n = len(tasks)
    out[:] = FILL
    assert L.emu_png_persp_color_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), rec.ctypes.data, n, 0) == 0
    assert (out == FILL).all()
    ok = color_task(good, dtype=0)
    assert L.emu_png_persp_color_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), rec.ctypes.data, 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 3].reshape(H, W, 3), WR.warp(EW._source(3, 8), (H, W), ident, WR.BILINEAR))

    # the label kernel
    lab = EW._label_sources()
    a, soff = EW._arena([lab[1], lab[2]])
    lbase = dict(src_off=soff[0], out_off=0, src_pitch=17, crop_w=17, crop_h=12, out_w=W, out_h=H, row0=0, rows=H, border_label=3,
                 src_bytes=1, dtype=3, border_mode=0)
    label_bad = [dict(out_w=0), dict(out_w=16385), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(row0=2, rows=H - 1), dict(crop_w=0),
                 dict(crop_h=0), dict(crop_h=1 << 31), dict(src_bytes=0), dict(src_bytes=3), dict(dtype=4),
                 dict(dtype=0, src_bytes=2, src_off=soff[1]), dict(border_mode=2), dict(src_bytes=2, src_off=soff[1] + 1)]

    def label_task(p, m=ident, **kw):
        t = EW.LabelWarpTask(**dict(lbase, **kw))
        t.m[:] = m
        return _persp(t, p)

    tasks = [label_task(good, **b) for b in label_bad] + [label_task(p) for p in bad_p] + [label_task(good, m=[1 << 32, 0, 0, 0, 65536, 0])]
    n = len(tasks)
    out = EW._aligned(4096 + H * W * 8 + 4096, FILL)
    assert L.emu_png_label_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), None, n, 0) == 0
    assert (out == FILL).all()
    ok = label_task(good)
    assert L.emu_png_label_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), None, 1, 0) == 0
    assert np.array_equal(out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W), WR.warp_labels(lab[1], (H, W), ident, WR.CONSTANT, 3))

    # the colour-label kernel
    rgb = ECL._sources()["blocky"]
    a = np.frombuffer(bytes(16) + rgb.tobytes(), np.uint8).copy()
    cl = dict(src_off=16, out_off=0, src_pitch=37, crop_w=37, crop_h=29, out_w=W, out_h=H, row0=0, rows=H, border_label=3, image=0,
              dtype=3, mode=0, border_mode=0)
    clbl_bad = [dict(out_w=0), dict(out_h=16385), dict(rows=0), dict(row0=H), dict(crop_w=0), dict(crop_h=1 << 31), dict(dtype=4),
                dict(mode=2), dict(border_mode=2), dict(dtype=1), dict(mode=1, map_slots=3), dict(mode=1, map_slots=8, map_off=8)]

    def clbl_task(p, **kw):
        return _persp(ECL._task(ident, **dict(cl, **kw)), p)

    tasks = [clbl_task(good, **b) for b in clbl_bad] + [clbl_task(p) for p in bad_p]
    n = len(tasks)
    out[:] = FILL
    cnt = np.zeros(1, np.uint32)
    tb = EW._aligned(64, 0)
    assert L.emu_png_color_label_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(tasks[0]) * n)(*tasks), tb.ctypes.data,
                                             cnt.ctypes.data, n, 0) == 0
    assert (out == FILL).all() and cnt[0] == 0
    ok = clbl_task(good)
    assert L.emu_png_color_label_persp_batch(a.ctypes.data, out.ctypes.data + 4096, (type(ok) * 1)(ok), tb.ctypes.data, None, 1, 0) == 0
    exp, _ = PR.warp_color_labels(rgb, (H, W), ident + good, WR.CONSTANT, 3, None, None, -1, "int64")
    assert np.array_equal(out[4096: 4096 + H * W * 8].view(np.int64).reshape(H, W), exp)


# ---- what the integer rule means ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [8, 16])
def test_uint_bilinear_against_the_rounded_float64_map(P):
    """the kernel's UINT bilinear result against floor(float64 + 1/2) at the exact position on the quantised matrix: within the
    bound derived in png_persp_ref's docstring (1 at P = 8, 6 at P = 16) -- and the bound is what the derivation says"""
    assert PR.float64_bound(8) == 1 and PR.float64_bound(16) == 6
    rng = np.random.default_rng(P)
    src = rng.integers(0, 1 << P, size=(23, 31, 2)).astype(np.uint8 if P == 8 else np.uint16)
    src[::3] = (1 << P) - 1  # full-scale steps: the largest |s01 - s00| the derivation allows for
    src[::3, ::2] = 0
    size = (40, 65)
    border = ((1 << P) - 1, 0, 0, 0)
    ms = matrices(31, 23, size)
    ms.update(keystones(31, 23, size, 4, seed=9))
    worst = 0
    for mode in (WR.CONSTANT, WR.CLAMP):
        got = run_persp([src], [(0, None, m) for m in ms.values()], size, "uint", "hwc", WR.BILINEAR, mode, border)
        for j, name in enumerate(ms):
            ref = np.floor(PR.warp_float64(src, size, ms[name], mode, border) + 0.5).astype(np.int64)
            diff = int(np.abs(got[j].astype(np.int64) - ref).max())
            worst = max(worst, diff)
            assert diff <= PR.float64_bound(P), (name, mode, diff)
    print(f"P = {P}: largest difference to the rounded float64 map {worst}, bound {PR.float64_bound(P)}")
