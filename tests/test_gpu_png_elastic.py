"""The elastic deformation on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_elastic, _labels_elastic,
_color_labels_elastic; api.png_decode_batch_tensor / _labels / _color_labels(..., elastic=)): the whole calls BIT FOR BIT against
the numpy restatement tests/png_elastic_ref.py applied to the reference decodes (png_out_format_ref, png_label_ref,
png_color_label_ref).  The batch is the seven small files of tests/test_gpu_png_warp.py -- RGB8 (67 x 41, the largest), RGBA8,
grey 16, a 4-bit palette file, an Adam7 file, one with a damaged CRC, and one that gets a node of 4097 pixels -- with a non-finite
node on one more; outputs of 1 x 1, 33 x 65 and 64 x 257 under grids of 2 x 2, 3 x 5 and 33 x 33 nodes; the order
E_LABEL > E_BOX > E_WARP > later errors; the slot of a failed file still holds `fill`; (a) no field and a field of zeros are
byte-identical to the call without elastic=, (b) a constant field of whole pixels is a translated warp=, through all three calls,
with and without warp= and with color=, tone= and blur=; (d) an image under NEAREST, its label map and its colour-coded mask
under one matrix and one field pick the same pixels."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_elastic_ref as ER  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402
import test_gpu_png_color_labels_warp as GCW  # noqa: E402  (the mask files and their maps)
import test_gpu_png_warp as GW  # noqa: E402  (the seven files, the affine matrices, the cached reference decodes)
from test_gpu_png_warp import api, files  # noqa: E402, F401  (fixtures)

pytestmark = pytest.mark.gpu
SIZES = GW.SIZES
GRIDS = [(2, 2), (3, 5), (33, 33)]  # (grid_h, grid_w), one per size
FILTERS, BORDERS = GW.FILTERS, GW.BORDERS
_np = GW._np
IDENT = (1, 0, 0, 0, 1, 0)


def _good_warps(api, file_list, size, seed):
    """GW._warps with a fine matrix on the last file (the fields carry the E_WARP cases here)"""
    ws = GW._warps(api, file_list, size, seed)
    ws[-1] = api.png_warp_matrix(file_list[-1][1], size, angle=20.0, scale=1.5)
    return ws


def _fields(n, grid, seed, amp=4.0, bad=(None, None)):
    """one field per file: none on file 1, zeros on file 2, random ones elsewhere; bad = (the file with a non-finite node, the
    file with a node of 4097 pixels)"""
    rng = np.random.default_rng(seed)
    fs = [rng.uniform(-amp, amp, size=grid + (2,)) for _ in range(n)]
    fs[1] = None
    fs[2] = np.zeros(grid + (2,))
    if bad[0] is not None:
        fs[bad[0]][-1, -1, 1] = math.nan
    if bad[1] is not None:
        fs[bad[1]][0, 0, 0] = 4097.0
    return fs


def _qm(M):
    return WR.quantise(IDENT if M is None else [v for r in M for v in r])


def _qf(F):
    return None if F is None else ER.quantise_field(F)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth,dtype", [("rgb", 8, "float32"), ("rgba", 16, "bfloat16"), ("rgb", 8, "uint"), ("gray_alpha", 16, "uint"),
                                              ("gray", 8, "float16")])
def test_tensor_elastic_mixed_batch(api, files, mode, depth, dtype, layout):
    datas = [d for d, _ in files]
    ch = GW.CH[mode]
    kw = dict(mean=GW.MEAN[:ch], std=GW.STD[:ch]) if dtype != "uint" else {}
    fill = 7 if dtype == "uint" else -3.0
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * ((1 << depth) - 1))) for x in bval] + [0] * (4 - ch)
    for k, size in enumerate(SIZES):
        grid = GRIDS[(k + depth // 8) % 3]
        ws = _good_warps(api, files, size, 10 * k + depth)
        fs = _fields(7, grid, 20 * k + depth, bad=(3 + k % 2, 6))
        for filt, bmode in (("bilinear", "constant"), ("nearest", "clamp")) if k % 2 == 0 else (("bilinear", "clamp"), ("nearest", "constant")):
            st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, fill=fill,
                                                       filter=filt, warp=ws, elastic=fs, border=bmode,
                                                       border_value=bval if bmode == "constant" else None, **kw)
            d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=False, **kw)[0]
            got = _np(t)
            assert got.shape == ((7, ch) + size if layout == "chw" else (7,) + size + (ch,))
            want_st = [ER.E_WARP if fs[i] is not None and _qf(fs[i]) is None else (R.E_CRC if i == 5 else 0) for i in range(7)]
            assert st == want_st and st.count(ER.E_WARP) == 2 and st.count(0) == 4, (st, want_st)
            sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == sentinel).all(), (i, "a failed file's slot was written")
                    continue
                rst, px, inf = GW._pixels(api, data, mode, depth)
                assert rst == 0 and infos[i] == inf
                want = ER.warp(px, size, _qm(ws[i]), _qf(fs[i]), FILTERS[filt], dtype, BORDERS[bmode], border, None, list(d.scale),
                               list(d.bias), layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (i, inf, size, grid, mode, depth, dtype, layout, filt, bmode, np.argwhere(got[i] != want)[:4])


@pytest.mark.parametrize("dtype,lut", [("int64", None), ("uint8", "lut"), ("int32", "lut"), ("uint16", None)])
def test_label_elastic_mixed_batch(api, files, dtype, lut):
    datas = [d for d, _ in files]
    table = None
    if lut:
        table = np.random.default_rng(9).permutation(256).astype(np.int64) - (0 if dtype == "uint8" else 100)
    g16 = LR.E_LABEL if dtype == "uint8" or lut else 0  # RGB8 and RGBA8 are no label files; grey 16 is none for uint8 or with a lut
    fill = 9
    for k, size in enumerate(SIZES):
        grid = GRIDS[k]
        ws = _good_warps(api, files, size, 50 + k)
        fs = _fields(7, grid, 60 + k, bad=(3 + k % 2, 6))
        fs[2] = np.random.default_rng(k).uniform(-3, 3, size=grid + (2,))  # (the grey 16 file is deformed too)
        for bmode, bl in (("constant", 255), ("constant", -1), ("clamp", None)):
            if bl == -1 and dtype in ("uint8", "uint16"):
                continue
            st, t, infos = api.png_decode_batch_labels(datas, size, dtype=dtype, lut=table, fill=fill, warp=ws, elastic=fs, border=bmode,
                                                       border_label=bl)
            got = _np(t)
            assert got.shape == (7,) + size and got.dtype == LR.DTYPES[dtype]
            want_st = [LR.E_LABEL, LR.E_LABEL, g16] + [ER.E_WARP if _qf(fs[i]) is None else (R.E_CRC if i == 5 else 0) for i in range(3, 7)]
            assert st == want_st and st.count(ER.E_WARP) == 2, (st, want_st)
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == fill).all(), (i, "a failed file's slot was written")
                    continue
                rst, lab, inf = GW._labels(data)
                assert rst == 0 and infos[i] == inf
                want = ER.warp_labels(lab, size, _qm(ws[i]), _qf(fs[i]), BORDERS[bmode], bl or 0, None, table, dtype)
                assert got[i].tobytes() == want.tobytes(), (i, inf, size, grid, dtype, bmode, bl, np.argwhere(got[i] != want)[:4])


@pytest.mark.parametrize("border", ["constant", "clamp"])
def test_color_label_elastic_mixed_batch(api, border):
    """the six mask files of the colour-label warp's test and a damaged one: PACK into int64, MAP into uint8 and int32 with the shared
    map, `unmatched` exact; a non-finite node and a node of 4097 are E_WARP, their slots and the damaged file's keep `fill`"""
    D = GCW._data()
    flist = D["files"] + [(GW._damage_crc(D["files"][0][0]), D["files"][0][1])]
    datas = [d for d, _ in flist]
    const = border == "constant"
    total = 0
    for k, size in enumerate(SIZES):
        grid = GRIDS[(k + 1) % 3]
        ws = GCW._warps(api, D["files"], size, 30 + k) + [None]
        fs = _fields(7, grid, 70 + k, bad=(2, 4))
        for dtype, maps, missing, bl in (("int64", None, -1, -100), ("uint8", GCW._values(D["keys"], "uint8"), 255, 255),
                                         ("int32", GCW._values(D["keys"], "int32"), -1, -1)):
            colors = None if maps is None else GCW._as_colors(maps)
            st, t, infos, um = api.png_decode_batch_color_labels(datas, size, colors, missing, dtype, fill=5, warp=ws, elastic=fs,
                                                                 border=border, border_label=bl if const else None)
            got = _np(t)
            assert st == [0, 0, ER.E_WARP, 0, ER.E_WARP, 0, R.E_CRC], st
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert um[i] == 0 and (got[i] == 5).all(), (i, "a failed file's slot was written")
                    continue
                rst, px, inf = GCW._ref(data)
                assert rst == 0 and infos[i] == inf
                exp, miss = ER.warp_color_labels(px, size, _qm(ws[i]), _qf(fs[i]), BORDERS[border], (bl if const else None) or 0, None, maps,
                                                 missing, dtype)
                assert got[i].tobytes() == exp.tobytes(), (i, inf, size, grid, dtype, border, np.argwhere(got[i] != exp)[:4])
                assert um[i] == miss, (i, um[i], miss)
                total += miss
    assert total > 0


def test_status_order_label_box_warp_then_later_errors(api, files):
    """one file per pair of neighbours in the order; every slot of a failed file keeps `fill`; nodes of exactly 4096 pixels pass"""
    rgb, g8 = files[0][0], files[6][0]
    crc = files[5][0]
    size, grid = (5, 6), (3, 5)
    ok = np.random.default_rng(3).uniform(-2, 2, size=grid + (2,))
    nan, big, edge = ok.copy(), ok.copy(), ok.copy()
    nan[0, 1, 0] = math.inf
    big[2, 2, 1] = -4097.0
    edge[1, 1] = (4096.0, -4096.0)
    datas = [rgb, rgb, g8, crc, g8[:60], g8, g8]
    boxes = [(0, 0, 68, 1), None, (0, 0, 10, 1), None, None, None, None]
    fs = [nan, big, big, nan, big, edge, ok]
    st, t, _ = api.png_decode_batch_labels(datas, size, dtype="int32", boxes=boxes, fill=-7, elastic=fs, border_label=-1)
    assert st == [LR.E_LABEL, LR.E_LABEL, LR.E_BOX, ER.E_WARP, ER.E_WARP, 0, 0]
    got = _np(t)
    assert (got[:5] == -7).all()
    fit = _qm(api.png_warp_matrix((9, 16), size))  # without warp=: the crop centred on the output
    for i in (5, 6):
        assert np.array_equal(got[i], ER.warp_labels(GW._labels(g8)[1], size, fit, _qf(fs[i]), ER.CONSTANT, -1, None, None, "int32")), i
    st, t, _ = api.png_decode_batch_tensor(datas, size, mode="gray", dtype="uint", boxes=boxes, fill=3, elastic=fs)
    assert st == [LR.E_BOX, ER.E_WARP, LR.E_BOX, ER.E_WARP, ER.E_WARP, 0, 0] and (_np(t)[:5] == 3).all()
    st, t, _, um = api.png_decode_batch_color_labels(datas, size, dtype="int32", boxes=boxes, fill=3, elastic=fs)
    assert st == [CR.E_BOX, ER.E_WARP, CR.E_BOX, ER.E_WARP, ER.E_WARP, 0, 0] and (_np(t)[:5] == 3).all() and um == [0] * 7
    # without the bad field the later errors show
    st, _, _ = api.png_decode_batch_labels([crc, g8[:60]], size, dtype="int32", elastic=[ok, None])
    assert st == [R.E_CRC, R.E_CHUNK]


def _moved(api, w, wh, size, a, b):
    """the matrix of property (b): w (None: the identity) with m02 + m00 a + m01 b and m12 + m10 a + m11 b"""
    m = np.array(((1.0, 0, 0), (0, 1.0, 0)) if w is None else w, dtype=np.float64)
    m[:, 2] += m[:, 0] * a + m[:, 1] * b
    return tuple(tuple(float(v) for v in r) for r in m)


def test_zero_and_constant_fields_are_byte_identical_to_warp(api, files):
    """(a) elastic=[None / zeros] against the same call without it, and (b) a constant field of whole pixels against the translated
    matrix (matrices rounded to multiples of 2^-16, where (b) is exact): through all three calls, with and without warp=, and with
    color=, tone= and blur="""
    import torch

    datas = [d for d, _ in files]
    n = len(datas)
    for k, size in enumerate(SIZES):
        grid = GRIDS[k]
        ws = [None if w is None else tuple(tuple(round(v * 65536) / 65536 for v in r) for r in w) for w in _good_warps(api, files, size, 90 + k)]
        fit = [api.png_warp_matrix(wh, size) for _, wh in files]
        zeros = [None if i % 2 else np.zeros(grid + (2,)) for i in range(n)]
        a, b = 3 - k, -2
        const = [np.broadcast_to(np.array([float(a), float(b)]), grid + (2,)) for _ in range(n)]
        extras = [dict(), dict(color=api.png_color_matrix(1.2, 0.8, 1.3, 17.0)), dict(tone=["equalize", ("posterize", 3), None, "autocontrast"] + [None] * (n - 4)),
                  dict(blur=[("gaussian", 5, 1.1), None, ("sharpness", 1.7)] + [None] * (n - 3)),
                  dict(color=api.png_color_matrix(0.9, 1.1, 0.7, -30.0), tone=[("solarize", 100)] * n, blur=[("gaussian", 3, 0.8)] * n)]
        for j, extra in enumerate(extras):
            kw = dict(mode="rgb", depth=8, dtype="float32" if j % 2 else "uint", layout="chw" if j % 2 else "hwc", fill=3,
                      filter="nearest" if (j + k) % 2 else "bilinear", border="constant" if j % 3 else "clamp", **extra)
            if kw["border"] == "constant":
                kw["border_value"] = (1.0, 0.5, 0.0)
            for base, given in ((ws, dict(warp=ws)), (fit, dict())):  # with warp=, and without (the matrix png_warp_matrix gives)
                plain = api.png_decode_batch_tensor(datas, size, warp=base, **kw)
                z = api.png_decode_batch_tensor(datas, size, elastic=zeros, **given, **kw)
                assert plain[0] == z[0] == [0, 0, 0, 0, 0, R.E_CRC, 0] and plain[2] == z[2]
                assert torch.equal(plain[1].view(torch.uint8), z[1].view(torch.uint8)), (size, j, list(given))
            moved = [_moved(api, w, wh, size, a, b) for w, (_, wh) in zip(ws, files)]
            m = api.png_decode_batch_tensor(datas, size, warp=moved, **kw)
            c = api.png_decode_batch_tensor(datas, size, warp=ws, elastic=const, **kw)
            assert m[0] == c[0] and torch.equal(m[1].view(torch.uint8), c[1].view(torch.uint8)), (size, j)
        for dtype, bl in (("int64", -1), ("uint16", 65535)):
            for base, given in ((ws, dict(warp=ws)), (fit, dict())):
                plain = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, warp=base, border_label=bl)
                z = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, elastic=zeros, border_label=bl, **given)
                assert plain[0] == z[0] and plain[2] == z[2] and torch.equal(plain[1].view(torch.uint8), z[1].view(torch.uint8)), (size, dtype)
            m = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, warp=moved, border_label=bl)
            c = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, warp=ws, elastic=const, border_label=bl)
            assert m[0] == c[0] and torch.equal(m[1].view(torch.uint8), c[1].view(torch.uint8)), (size, dtype)
    D = GCW._data()
    cdatas = [d for d, _ in D["files"]]
    for k, size in enumerate(GCW.SIZES):
        grid = GRIDS[k % 3]
        ws = GCW._warps(api, D["files"], size, 30 + k)
        fit = [api.png_warp_matrix(wh, size) for _, wh in D["files"]]
        zeros = [None if i % 2 else np.zeros(grid + (2,)) for i in range(6)]
        for colors, dtype, missing in ((None, "int32", -1), (GCW._as_colors(GCW._values(D["keys"], "uint8")), "uint8", 255)):
            bl = missing if dtype == "uint8" else -9
            for base, given in ((ws, dict(warp=ws)), (fit, dict())):
                plain = api.png_decode_batch_color_labels(cdatas, size, colors, missing, dtype, warp=base, border_label=bl)
                z = api.png_decode_batch_color_labels(cdatas, size, colors, missing, dtype, elastic=zeros, border_label=bl, **given)
                assert plain[0] == z[0] == [0] * 6 and plain[2] == z[2] and plain[3] == z[3]
                assert torch.equal(plain[1].view(torch.uint8), z[1].view(torch.uint8)), (size, dtype)


def test_image_label_map_and_colour_mask_pick_the_same_source_pixels(api):
    """(d) three files of one picture: a palette file whose index names the pixel (y * 16 + x) and whose PLTE entry i is
    (i % 16, i // 16, 0) -- the image call sees its own coordinates in R and G, the label call in the index, the colour-label call in
    the packed colour R | G << 8 --; under one matrix and one field per file all three name the same pixel, or all three the border"""
    rng = np.random.default_rng(78)
    yy, xx = np.mgrid[0:15, 0:16]
    idx = (yy * 16 + xx).astype(np.uint8)[:, :, None]
    pal = [(i % 16, i // 16, 0) for i in range(256)]
    datas = [R.encode(idx[: 15 - k, : 16 - 2 * k], 3, 8, k % 2, palette=pal) for k in range(6)]
    size = (33, 65)
    for grid, with_warp in (((3, 5), True), ((33, 33), False)):
        ws = [api.png_warp_matrix((16 - 2 * k, 15 - k), size, angle=25.0 * k - 40, scale=(65 / 16 * 0.8, 33 / 15 * 0.8)) for k in range(6)]
        given = dict(warp=ws) if with_warp else {}
        fs = [rng.uniform(-5, 5, size=grid + (2,)) for _ in range(6)]
        for bmode in ("constant", "clamp"):
            const = bmode == "constant"
            st, img, _ = api.png_decode_batch_tensor(datas, size, mode="rgb", dtype="uint", layout="hwc", filter="nearest", elastic=fs,
                                                     border=bmode, border_value=(1.0, 1.0, 1.0) if const else None, **given)
            st2, lab, _ = api.png_decode_batch_labels(datas, size, dtype="int32", elastic=fs, border=bmode,
                                                      border_label=-1 if const else None, **given)
            st3, clb, _, _ = api.png_decode_batch_color_labels(datas, size, dtype="int32", elastic=fs, border=bmode,
                                                               border_label=-1 if const else None, **given)
            assert st == st2 == st3 == [0] * 6
            img, lab, clb = _np(img).astype(np.int32), _np(lab), _np(clb)
            outside = lab == -1
            assert np.array_equal(outside, img[:, :, :, 0] == 255) and np.array_equal(outside, clb == -1)
            assert outside.any() == const and (~outside).any()
            assert np.array_equal(lab[~outside], (img[:, :, :, 1] * 16 + img[:, :, :, 0])[~outside])
            assert np.array_equal((lab // 16 * 256 + lab % 16)[~outside], clb[~outside])
            # and they are the restatement's picks
            for k in range(6):
                m = _qm(ws[k] if with_warp else api.png_warp_matrix((16 - 2 * k, 15 - k), size))
                want = ER.warp_labels(idx[: 15 - k, : 16 - 2 * k, 0], size, m, _qf(fs[k]), BORDERS[bmode], -1, None, None, "int32")
                assert np.array_equal(lab[k], want), (grid, bmode, k)
