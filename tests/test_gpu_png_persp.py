"""The perspective warp on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_persp, _labels_persp,
_color_labels_persp; api.png_decode_batch_tensor / _labels / _color_labels(..., perspective=)): the whole calls BIT FOR BIT against
the numpy restatement tests/png_persp_ref.py applied to the reference decodes (png_out_format_ref, png_label_ref,
png_color_label_ref).  The batch is the seven small files of tests/test_gpu_png_warp.py -- RGB8 (67 x 41, the largest), RGBA8,
grey 16, a 4-bit palette file, an Adam7 file, one with a damaged CRC, and one that gets a non-finite matrix -- with a horizon through
the output on one more; outputs of 1 x 1, 33 x 65 and 64 x 257; the order E_LABEL > E_BOX > E_WARP > later errors; the slot of a
failed file still holds `fill`; affine matrices through perspective= are byte-identical to warp= through all three calls and with
color=, tone= and blur=; an image under NEAREST, its label map and its colour-coded mask under one random homography pick the same
pixels."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_label_ref as CR  # noqa: E402
import png_label_ref as LR  # noqa: E402
import png_persp_ref as PR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_emu_png_persp as EP  # noqa: E402  (the keystone generator)
import test_gpu_png_color_labels_warp as GCW  # noqa: E402  (the mask files and their maps)
import test_gpu_png_warp as GW  # noqa: E402  (the seven files, the affine matrices, the cached reference decodes)
from test_gpu_png_warp import api, files  # noqa: E402, F401  (fixtures)

pytestmark = pytest.mark.gpu
SIZES = GW.SIZES
NAN = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, math.nan, 1.0))
FILTERS, BORDERS = GW.FILTERS, GW.BORDERS
_np = GW._np


def _horizon(size):
    """D = 1 - 2 (X + 1/2) / W: zero or negative from the middle column on, at every size"""
    return ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-2.0 / size[1], 0.0, 1.0))


def _maps(file_list, size, seed, bad=True, boxes=None):
    """one 3 x 3 matrix per file: the identity (None), then random keystones; with `bad`: the horizon on file 3 or 4, the non-finite
    matrix on file 6"""
    rng = np.random.default_rng(seed)
    ms = []
    for k, (_, wh) in enumerate(file_list):
        if boxes is not None and boxes[k] is not None:
            wh = boxes[k][2:]
        ms.append(None if k == 0 else EP.keystone(wh[0], wh[1], size, rng)[0])
    if bad:
        ms[3 + seed % 2] = _horizon(size)
        ms[6] = NAN
    return ms


def _q(M):
    return PR.quantise(PR_IDENT if M is None else [v for r in M for v in r])


PR_IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)


def _want_status(M, size, otherwise=0):
    m = _q(M)
    return otherwise if m is not None and PR.range_ok(m, size) else PR.E_WARP


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth,dtype", [("rgb", 8, "float32"), ("rgba", 16, "bfloat16"), ("rgb", 8, "uint"), ("gray_alpha", 16, "uint"),
                                              ("gray", 8, "float16")])
def test_tensor_persp_mixed_batch(api, files, mode, depth, dtype, layout):
    datas = [d for d, _ in files]
    ch = GW.CH[mode]
    kw = dict(mean=GW.MEAN[:ch], std=GW.STD[:ch]) if dtype != "uint" else {}
    fill = 7 if dtype == "uint" else -3.0
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * ((1 << depth) - 1))) for x in bval] + [0] * (4 - ch)
    for k, size in enumerate(SIZES):
        ms = _maps(files, size, 10 * k + depth + k)
        for filt, bmode in (("bilinear", "constant"), ("nearest", "clamp")) if k % 2 == 0 else (("bilinear", "clamp"), ("nearest", "constant")):
            st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, fill=fill,
                                                       filter=filt, perspective=ms, border=bmode,
                                                       border_value=bval if bmode == "constant" else None, **kw)
            d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=False, **kw)[0]
            got = _np(t)
            assert got.shape == ((7, ch) + size if layout == "chw" else (7,) + size + (ch,))
            want_st = [_want_status(ms[i], size, R.E_CRC if i == 5 else 0) for i in range(7)]
            assert st == want_st and st.count(PR.E_WARP) == 2 and st.count(0) == 4, (st, want_st)
            sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == sentinel).all(), (i, "a failed file's slot was written")
                    continue
                rst, px, inf = GW._pixels(api, data, mode, depth)
                assert rst == 0 and infos[i] == inf
                want = PR.warp(px, size, _q(ms[i]), FILTERS[filt], dtype, BORDERS[bmode], border, None, list(d.scale), list(d.bias), layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (i, inf, size, mode, depth, dtype, layout, filt, bmode, np.argwhere(got[i] != want)[:4])


@pytest.mark.parametrize("dtype,lut", [("int64", None), ("uint8", "lut"), ("int32", "lut"), ("uint16", None)])
def test_label_persp_mixed_batch(api, files, dtype, lut):
    datas = [d for d, _ in files]
    table = None
    if lut:
        table = np.random.default_rng(9).permutation(256).astype(np.int64) - (0 if dtype == "uint8" else 100)
    g16 = LR.E_LABEL if dtype == "uint8" or lut else 0  # RGB8 and RGBA8 are no label files; grey 16 is none for uint8 or with a lut
    fill = 9
    for k, size in enumerate(SIZES):
        ms = _maps(files, size, 50 + k)
        for bmode, bl in (("constant", 255), ("constant", -1), ("clamp", None)):
            if bl == -1 and dtype in ("uint8", "uint16"):
                continue
            st, t, infos = api.png_decode_batch_labels(datas, size, dtype=dtype, lut=table, fill=fill, perspective=ms, border=bmode,
                                                       border_label=bl)
            got = _np(t)
            assert got.shape == (7,) + size and got.dtype == LR.DTYPES[dtype]
            want_st = [LR.E_LABEL, LR.E_LABEL, g16] + [_want_status(ms[i], size, R.E_CRC if i == 5 else 0) for i in range(3, 7)]
            assert st == want_st and st.count(PR.E_WARP) == 2, (st, want_st)
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == fill).all(), (i, "a failed file's slot was written")
                    continue
                rst, lab, inf = GW._labels(data)
                assert rst == 0 and infos[i] == inf
                want = PR.warp_labels(lab, size, _q(ms[i]), BORDERS[bmode], bl or 0, None, table, dtype)
                assert got[i].tobytes() == want.tobytes(), (i, inf, size, dtype, bmode, bl, np.argwhere(got[i] != want)[:4])


@pytest.mark.parametrize("border", ["constant", "clamp"])
def test_color_label_persp_mixed_batch(api, border):
    """the six mask files of the colour-label warp's test and a damaged one: PACK into int64, MAP into uint8 and int32 with the shared
    map, `unmatched` exact; a horizon and a non-finite matrix are E_WARP, their slots and the damaged file's keep `fill`"""
    D = GCW._data()
    flist = D["files"] + [(GW._damage_crc(D["files"][0][0]), D["files"][0][1])]
    datas = [d for d, _ in flist]
    const = border == "constant"
    total = 0
    for k, size in enumerate(SIZES):
        ms = _maps(flist, size, 70 + k, bad=False)
        ms[2], ms[4] = _horizon(size), NAN
        for dtype, maps, missing, bl in (("int64", None, -1, -100), ("uint8", GCW._values(D["keys"], "uint8"), 255, 255),
                                         ("int32", GCW._values(D["keys"], "int32"), -1, -1)):
            colors = None if maps is None else GCW._as_colors(maps)
            st, t, infos, um = api.png_decode_batch_color_labels(datas, size, colors, missing, dtype, fill=5, perspective=ms, border=border,
                                                                 border_label=bl if const else None)
            got = _np(t)
            assert st == [0, 0, PR.E_WARP, 0, PR.E_WARP, 0, R.E_CRC], st
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert um[i] == 0 and (got[i] == 5).all(), (i, "a failed file's slot was written")
                    continue
                rst, px, inf = GCW._ref(data)
                assert rst == 0 and infos[i] == inf
                exp, miss = PR.warp_color_labels(px, size, _q(ms[i]), BORDERS[border], (bl if const else None) or 0, None, maps, missing, dtype)
                assert got[i].tobytes() == exp.tobytes(), (i, inf, size, dtype, border, np.argwhere(got[i] != exp)[:4])
                assert um[i] == miss, (i, um[i], miss)
                total += miss
    assert total > 0


def test_status_order_label_box_warp_then_later_errors(api, files):
    """one file per pair of neighbours in the order; every slot of a failed file keeps `fill`"""
    rgb, g8 = files[0][0], files[6][0]
    crc = files[5][0]
    size = (5, 6)
    H = _horizon(size)
    datas = [rgb, rgb, g8, crc, g8[:60], g8, g8]
    boxes = [(0, 0, 68, 1), None, (0, 0, 10, 1), None, None, None, None]
    ms = [NAN, H, H, H, NAN, None, EP.keystone(9, 16, size, np.random.default_rng(1))[0]]
    st, t, _ = api.png_decode_batch_labels(datas, size, dtype="int32", boxes=boxes, fill=-7, perspective=ms, border_label=-1)
    assert st == [LR.E_LABEL, LR.E_LABEL, LR.E_BOX, PR.E_WARP, PR.E_WARP, 0, 0]
    got = _np(t)
    assert (got[:5] == -7).all()
    for i in (5, 6):
        assert np.array_equal(got[i], PR.warp_labels(GW._labels(g8)[1], size, _q(ms[i]), PR.CONSTANT, -1, None, None, "int32")), i
    st, t, _ = api.png_decode_batch_tensor(datas, size, mode="gray", dtype="uint", boxes=boxes, fill=3, perspective=ms)
    assert st == [LR.E_BOX, PR.E_WARP, LR.E_BOX, PR.E_WARP, PR.E_WARP, 0, 0] and (_np(t)[:5] == 3).all()
    st, t, _, um = api.png_decode_batch_color_labels(datas, size, dtype="int32", boxes=boxes, fill=3, perspective=ms)
    assert st == [CR.E_BOX, PR.E_WARP, CR.E_BOX, PR.E_WARP, PR.E_WARP, 0, 0] and (_np(t)[:5] == 3).all() and um == [0] * 7
    # without the bad matrix the later errors show
    st, _, _ = api.png_decode_batch_labels([crc, g8[:60]], size, dtype="int32", perspective=[None, None])
    assert st == [R.E_CRC, R.E_CHUNK]


def test_affine_matrices_are_byte_identical_to_warp(api, files):
    """perspective=png_perspective_from_warp(m) against warp=m: through all three calls, and with color=, tone= and blur="""
    import torch

    datas = [d for d, _ in files]
    for k, size in enumerate(SIZES):
        ws = GW._warps(api, files, size, 90 + k)
        ps = [None if w is None else api.png_perspective_from_warp(w) for w in ws[:6]] + [NAN]
        n = len(datas)
        extras = [dict(), dict(color=api.png_color_matrix(1.2, 0.8, 1.3, 17.0)), dict(tone=["equalize", ("posterize", 3), None, "autocontrast"] + [None] * (n - 4)),
                  dict(blur=[("gaussian", 5, 1.1), None, ("sharpness", 1.7)] + [None] * (n - 3)),
                  dict(color=api.png_color_matrix(0.9, 1.1, 0.7, -30.0), tone=[("solarize", 100)] * n, blur=[("gaussian", 3, 0.8)] * n)]
        for j, extra in enumerate(extras):
            kw = dict(mode="rgb", depth=8, dtype="float32" if j % 2 else "uint", layout="chw" if j % 2 else "hwc", fill=3,
                      filter="nearest" if (j + k) % 2 else "bilinear", border="constant" if j % 3 else "clamp", **extra)
            if kw["border"] == "constant":
                kw["border_value"] = (1.0, 0.5, 0.0)
            a = api.png_decode_batch_tensor(datas, size, warp=ws, **kw)
            b = api.png_decode_batch_tensor(datas, size, perspective=ps, **kw)
            assert a[0] == b[0] == [0, 0, 0, 0, 0, R.E_CRC, PR.E_WARP] and a[2] == b[2]
            assert torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8)), (size, j)
        for dtype, bl in (("int64", -1), ("uint16", 65535)):
            a = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, warp=ws, border_label=bl)
            b = api.png_decode_batch_labels(datas, size, dtype=dtype, fill=9, perspective=ps, border_label=bl)
            assert a[0] == b[0] and a[2] == b[2] and torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8)), (size, dtype)
    D = GCW._data()
    cdatas = [d for d, _ in D["files"]]
    for k, size in enumerate(GCW.SIZES):
        ws = GCW._warps(api, D["files"], size, 30 + k)
        ps = [None if w is None else api.png_perspective_from_warp(w) for w in ws]
        for colors, dtype, missing in ((None, "int32", -1), (GCW._as_colors(GCW._values(D["keys"], "uint8")), "uint8", 255)):
            a = api.png_decode_batch_color_labels(cdatas, size, colors, missing, dtype, warp=ws, border_label=missing if dtype == "uint8" else -9)
            b = api.png_decode_batch_color_labels(cdatas, size, colors, missing, dtype, perspective=ps, border_label=missing if dtype == "uint8" else -9)
            assert a[0] == b[0] == [0] * 6 and a[2] == b[2] and a[3] == b[3] and torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8)), (size, dtype)


def test_image_label_map_and_colour_mask_pick_the_same_source_pixels(api):
    """three files of one picture: a palette file whose index names the pixel (y * 16 + x) and whose PLTE entry i is
    (i % 16, i // 16, 0) -- the image call sees its own coordinates in R and G, the label call in the index, the colour-label call in
    the packed colour R | G << 8 --; under one random homography per file all three name the same pixel, or all three the border"""
    rng = np.random.default_rng(78)
    yy, xx = np.mgrid[0:15, 0:16]
    idx = (yy * 16 + xx).astype(np.uint8)[:, :, None]
    pal = [(i % 16, i // 16, 0) for i in range(256)]
    datas = [R.encode(idx[: 15 - k, : 16 - 2 * k], 3, 8, k % 2, palette=pal) for k in range(6)]
    size = (33, 65)
    ms = [EP.keystone(16 - 2 * k, 15 - k, size, rng)[0] for k in range(6)]
    for bmode in ("constant", "clamp"):
        const = bmode == "constant"
        st, img, _ = api.png_decode_batch_tensor(datas, size, mode="rgb", dtype="uint", layout="hwc", filter="nearest", perspective=ms,
                                                 border=bmode, border_value=(1.0, 1.0, 1.0) if const else None)
        st2, lab, _ = api.png_decode_batch_labels(datas, size, dtype="int32", perspective=ms, border=bmode, border_label=-1 if const else None)
        st3, clb, _, _ = api.png_decode_batch_color_labels(datas, size, dtype="int32", perspective=ms, border=bmode,
                                                           border_label=-1 if const else None)
        assert st == st2 == st3 == [0] * 6
        img, lab, clb = _np(img).astype(np.int32), _np(lab), _np(clb)
        outside = lab == -1
        assert np.array_equal(outside, img[:, :, :, 0] == 255) and np.array_equal(outside, clb == -1)
        assert outside.any() == const and (~outside).any()
        assert np.array_equal(lab[~outside], (img[:, :, :, 1] * 16 + img[:, :, :, 0])[~outside])
        assert np.array_equal((lab // 16 * 256 + lab % 16)[~outside], clb[~outside])
