"""The affine warp on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_warp, debig_png_decode_batch_labels_warp;
api.png_decode_batch_tensor(..., warp=), api.png_decode_batch_labels(..., warp=)): the whole calls BIT FOR BIT against the numpy
restatement tests/png_warp_ref.py applied to the decodes of tests/png_spec_ref.py (through png_out_format_ref.decode) and
tests/png_label_ref.py.  Batches of seven small files -- RGB8 (67 x 41, the largest), RGBA8, grey 16, a 4-bit palette file, an
Adam7 file, one with a damaged CRC and one with an E_WARP matrix --, outputs of 1 x 1, 33 x 65 and 64 x 257, both layouts,
float32 / bfloat16 / uint, both filters and border modes; the slot of a failed file still holds `fill`; the order
E_LABEL > E_BOX > E_WARP > later errors; an image and its label map under one random matrix pick the same source pixels."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_out_format_ref as F  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (33, 65), (64, 257)]  # (H, W)
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3, "gray": 1, "gray_alpha": 2}
NAN = ((1.0, 0.0, math.nan), (0.0, 1.0, 0.0))
FILTERS = {"bilinear": WR.BILINEAR, "nearest": WR.NEAREST}
BORDERS = {"constant": WR.CONSTANT, "clamp": WR.CLAMP}


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


def _damage_crc(data):
    b = bytearray(data)
    b[-20] ^= 1  # inside the last IDAT's payload: its CRC no longer matches
    return bytes(b)


@pytest.fixture(scope="module")
def files():
    """[(data, (w, h))]: RGB8, RGBA8, grey 16, palette 4-bit, grey 8 Adam7, grey 8 with a damaged CRC, grey 8 (it gets the
    E_WARP matrix)"""
    rng = np.random.default_rng(2026)
    ft = lambda p, y: y % 5  # noqa: E731
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(11)]
    specs = [(67, 41, 2, 8, 0, None), (40, 33, 6, 8, 0, None), (45, 30, 0, 16, 0, None), (33, 17, 3, 4, 0, pal), (21, 19, 0, 8, 1, None),
             (16, 9, 0, 8, 0, None), (9, 16, 0, 8, 0, None)]
    out = []
    for w, h, ct, depth, il, p in specs:
        s = R.random_image(rng, w, h, ct, depth, len(p) if p else None)
        out.append((R.encode(s, ct, depth, il, palette=p, filters=ft), (w, h)))
    out[5] = (_damage_crc(out[5][0]), out[5][1])
    return out


def _warps(api, files, size, seed):
    """one matrix per file: the identity (None), a flip, a quarter turn, random rotations / scales / shears / translations"""
    rng = np.random.default_rng(seed)
    ws = []
    for k, (_, wh) in enumerate(files):
        if k == 0:
            ws.append(None)
        elif k == 1:
            ws.append(api.png_warp_matrix(wh, size, hflip=True, angle=90))
        else:
            ws.append(api.png_warp_matrix(wh, size, angle=float(rng.uniform(-180, 180)), scale=float(rng.uniform(0.5, 6.0)),
                                          shear=(float(rng.uniform(-15, 15)), float(rng.uniform(-15, 15))),
                                          translate=(float(rng.uniform(-4, 4)), float(rng.uniform(-4, 4))), vflip=bool(k % 2)))
    ws[6] = NAN
    return ws


def _q(m):
    return WR.quantise((1, 0, 0, 0, 1, 0) if m is None else [v for r in m for v in r])


def _np(t):
    import torch

    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


_PX = {}


def _pixels(api, data, mode, depth):
    """the restatement's decode of a file in the tensor's format, computed once"""
    if (data, mode, depth) not in _PX:
        _PX[(data, mode, depth)] = F.decode(data, api.png_out_format(mode, depth))
    return _PX[(data, mode, depth)]


_LAB = {}


def _labels(data):
    if data not in _LAB:
        _LAB[data] = LR.labels(data)
    return _LAB[data]


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth,dtype", [("rgb", 8, "float32"), ("rgba", 16, "bfloat16"), ("rgb", 8, "uint"), ("gray_alpha", 16, "uint"),
                                              ("gray", 8, "float16")])
def test_tensor_warp_mixed_batch(api, files, mode, depth, dtype, layout):
    datas = [d for d, _ in files]
    ch = CH[mode]
    kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
    fill = 7 if dtype == "uint" else -3.0
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * ((1 << depth) - 1))) for x in bval] + [0] * (4 - ch)
    for k, size in enumerate(SIZES):
        ws = _warps(api, files, size, 10 * k + depth)
        for filt, bmode in (("bilinear", "constant"), ("nearest", "clamp")) if k % 2 == 0 else (("bilinear", "clamp"), ("nearest", "constant")):
            st, t, infos = api.png_decode_batch_tensor(datas, size, mode=mode, depth=depth, dtype=dtype, layout=layout, fill=fill,
                                                       filter=filt, warp=ws, border=bmode,
                                                       border_value=bval if bmode == "constant" else None, **kw)
            d = api.png_tensor_desc(size, mode, depth, dtype, layout, antialias=False, **kw)[0]
            got = _np(t)
            assert got.shape == ((7, ch) + size if layout == "chw" else (7,) + size + (ch,))
            assert st == [0, 0, 0, 0, 0, R.E_CRC, WR.E_WARP], st
            sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == sentinel).all(), (i, "a failed file's slot was written")
                    continue
                rst, px, inf = _pixels(api, data, mode, depth)
                assert rst == 0 and infos[i] == inf
                want = WR.warp(px, size, _q(ws[i]), FILTERS[filt], dtype, BORDERS[bmode], border, None, list(d.scale), list(d.bias), layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (i, inf, size, mode, depth, dtype, layout, filt, bmode, np.argwhere(got[i] != want)[:4])


def test_identity_flips_and_quarter_turns_of_real_files_with_boxes(api, files):
    """out == crop: the warp call with the flip / turn matrices is numpy.flip / numpy.rot90 of the cropped decode, both filters"""
    datas = [d for d, _ in files[:5]]
    box = (3, 2, 17, 13)
    turns = {"identity": lambda d: d, "hflip": lambda d: np.flip(d, 1), "vflip": lambda d: np.flip(d, 0),
             "rot90": lambda d: np.rot90(d, 1), "rot180": lambda d: np.rot90(d, 2), "rot270": lambda d: np.rot90(d, 3)}
    kws = {"identity": {}, "hflip": dict(hflip=True), "vflip": dict(vflip=True), "rot90": dict(angle=90), "rot180": dict(angle=180),
           "rot270": dict(angle=270)}
    for name, fn in turns.items():
        size = (17, 13) if name in ("rot90", "rot270") else (13, 17)
        m = api.png_warp_matrix((17, 13), size, **kws[name])
        for filt in ("bilinear", "nearest"):
            st, t, _ = api.png_decode_batch_tensor(datas, size, mode="rgba", depth=16, dtype="uint", layout="hwc", boxes=[box] * 5,
                                                   filter=filt, warp=[m] * 5)
            assert st == [0] * 5
            for i, data in enumerate(datas):
                px = _pixels(api, data, "rgba", 16)[1][2:15, 3:20]
                assert np.array_equal(_np(t)[i], fn(px)), (name, filt, i)


@pytest.mark.parametrize("dtype,lut", [("int64", None), ("uint8", "lut"), ("int32", "lut"), ("uint16", None)])
def test_label_warp_mixed_batch(api, files, dtype, lut):
    datas = [d for d, _ in files]
    table = None
    if lut:
        table = np.random.default_rng(9).permutation(256).astype(np.int64) - (0 if dtype == "uint8" else 100)
    # RGB8 and RGBA8 are no label files; grey 16 is none for uint8 or with a lut
    g16 = LR.E_LABEL if dtype == "uint8" or lut else 0
    fill = 9
    for k, size in enumerate(SIZES):
        ws = _warps(api, files, size, 50 + k)
        for bmode, bl in (("constant", 255), ("constant", -1), ("clamp", None)):
            if bl == -1 and dtype in ("uint8", "uint16"):
                continue
            st, t, infos = api.png_decode_batch_labels(datas, size, dtype=dtype, lut=table, fill=fill, warp=ws, border=bmode, border_label=bl)
            got = _np(t)
            assert got.shape == (7,) + size and got.dtype == LR.DTYPES[dtype]
            assert st == [LR.E_LABEL, LR.E_LABEL, g16, 0, 0, R.E_CRC, WR.E_WARP], st
            for i, data in enumerate(datas):
                if st[i] != 0:
                    assert (got[i] == fill).all(), (i, "a failed file's slot was written")
                    continue
                rst, lab, inf = _labels(data)
                assert rst == 0 and infos[i] == inf
                want = WR.warp_labels(lab, size, _q(ws[i]), BORDERS[bmode], bl or 0, None, table, dtype)
                assert got[i].tobytes() == want.tobytes(), (i, inf, size, dtype, bmode, bl, np.argwhere(got[i] != want)[:4])


def test_status_order_label_box_warp_then_later_errors(api, files):
    """one file per pair of neighbours in the order; every slot of a failed file keeps `fill`"""
    rgb, g8 = files[0][0], files[6][0]
    crc = files[5][0]
    datas = [rgb, rgb, g8, crc, g8[:60], g8]
    boxes = [(0, 0, 68, 1), None, (0, 0, 10, 1), None, None, None]
    ws = [NAN, NAN, NAN, NAN, NAN, None]
    st, t, _ = api.png_decode_batch_labels(datas, (5, 6), dtype="int32", boxes=boxes, fill=-7, warp=ws, border_label=-1)
    assert st == [LR.E_LABEL, LR.E_LABEL, LR.E_BOX, WR.E_WARP, WR.E_WARP, 0]
    got = _np(t)
    assert (got[:5] == -7).all()
    assert np.array_equal(got[5], WR.warp_labels(_labels(g8)[1], (5, 6), _q(None), WR.CONSTANT, -1, None, None, "int32"))
    st, t, _ = api.png_decode_batch_tensor(datas, (5, 6), mode="gray", dtype="uint", boxes=boxes, fill=3, warp=ws)
    assert st == [LR.E_BOX, WR.E_WARP, LR.E_BOX, WR.E_WARP, WR.E_WARP, 0] and (_np(t)[:5] == 3).all()
    # without the bad matrix the later errors show
    st, _, _ = api.png_decode_batch_labels([crc, g8[:60]], (5, 6), dtype="int32", warp=[None, None])
    assert st == [R.E_CRC, R.E_CHUNK]


def test_image_and_label_pick_the_same_source_pixels(api):
    """a palette file whose PLTE entry i is (x, y) of the pixels that carry index i... reversed: the INDEX of pixel (x, y) is
    y * 16 + x and PLTE entry i is (i % 16, i // 16, 0), so the image names its own coordinates in R and G and the label map
    names them in its value; under one random matrix per file both calls must name the same pixel, or both the border"""
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:15, 0:16]
    idx = (yy * 16 + xx).astype(np.uint8)[:, :, None]
    pal = [(i % 16, i // 16, 0) for i in range(256)]
    datas = [R.encode(idx[: 15 - k, : 16 - 2 * k], 3, 8, k % 2, palette=pal) for k in range(6)]
    size = (33, 65)
    ws = [api.png_warp_matrix((16 - 2 * k, 15 - k), size, angle=float(rng.uniform(-180, 180)), scale=float(rng.uniform(1.0, 5.0)),
                              shear=(float(rng.uniform(-10, 10)), 0.0), translate=(float(rng.uniform(-9, 9)), float(rng.uniform(-5, 5))),
                              hflip=bool(k & 1), vflip=bool(k & 2)) for k in range(6)]
    for bmode in ("constant", "clamp"):
        st, img, _ = api.png_decode_batch_tensor(datas, size, mode="rgb", dtype="uint", layout="hwc", filter="nearest", warp=ws,
                                                 border=bmode, border_value=(1.0, 1.0, 1.0) if bmode == "constant" else None)
        st2, lab, _ = api.png_decode_batch_labels(datas, size, dtype="int32", warp=ws, border=bmode,
                                                  border_label=-1 if bmode == "constant" else None)
        assert st == st2 == [0] * 6
        img, lab = _np(img).astype(np.int32), _np(lab)
        outside = lab == -1
        assert np.array_equal(outside, img[:, :, :, 0] == 255)
        assert bmode == "constant" or not outside.any()
        assert outside.any() == (bmode == "constant") and (~outside).any()
        assert np.array_equal(lab[~outside], (img[:, :, :, 1] * 16 + img[:, :, :, 0])[~outside])
