"""The per-image colour matrix on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_color,
debig_png_decode_batch_tensor_warp_color; api.png_decode_batch_tensor(..., color=)): the whole calls BIT FOR BIT against the numpy
restatement tests/png_color_ref.py applied to the decodes of tests/png_spec_ref.py (through png_out_format_ref.decode).  One batch
of six small files -- RGB8 70 x 37, RGBA8 70 x 37, RGB16 33 x 21, a 4-bit palette file with tRNS 19 x 9, one with a damaged CRC and
one whose matrix holds a NaN --, every file with a matrix of its own; resized to 67 x 19 (two tiles in x, an odd width for the CHW
byte stores) and warped to 67 x 70 (more than one 4096-pixel task); every dtype, both layouts, modes rgb and rgba, 8 and 16 bits.
The slot of a failed file still holds `fill`.  The exact consequences of the rule are asserted on their own."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_ref as CR  # noqa: E402
import png_out_format_ref as F  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
RESIZE_TO, WARP_TO = (19, 67), (70, 67)  # (H, W)
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3}
DTYPES = ["uint", "float32", "float16", "bfloat16"]
N_OK = 4


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def files():
    """[(data, (w, h))]: RGB8, RGBA8, RGB16, palette 4-bit with tRNS, RGB8 with a damaged CRC, RGB8 (it gets the NaN matrix)"""
    rng = np.random.default_rng(2027)
    ft = lambda p, y: y % 5  # noqa: E731
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(13)]
    trns = bytes(int(v) for v in rng.integers(0, 256, 9))
    specs = [(70, 37, 2, 8, None, None), (70, 37, 6, 8, None, None), (33, 21, 2, 16, None, None), (19, 9, 3, 4, pal, trns),
             (16, 9, 2, 8, None, None), (9, 16, 2, 8, None, None)]
    out = []
    for w, h, ct, depth, p, t in specs:
        s = R.random_image(rng, w, h, ct, depth, len(p) if p else None)
        out.append((R.encode(s, ct, depth, 0, trns=t, palette=p, filters=ft), (w, h)))
    b = bytearray(out[4][0])
    b[-20] ^= 1  # inside the last IDAT's payload: its CRC no longer matches
    out[4] = (bytes(b), out[4][1])
    return out


def _matrices(api):
    """one per file, all different (reading another image's record shows); the last one holds a NaN"""
    nan = np.array(CR.IDENTITY)
    nan[1, 2] = math.nan
    return np.stack([api.png_color_matrix(1.2, 0.8, 1.3, 17.0), api.png_color_matrix(0.7, 1.4, 0.2, -60.0),
                     np.array([[2.0, -1.5, 0.7, -0.1], [-0.6, 1.9, -0.4, 0.3], [0.2, 0.4, -2.0, 1.1]]),
                     np.array([[16.0, -16.0, 16.0, -16.0], [-16.0, 16.0, -16.0, 16.0], [0.001, -0.002, 0.003, 0.5]]),
                     api.png_color_matrix(saturation=0.0), nan])


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


def _check_failed(st, got, fill, dtype):
    assert st == [0] * N_OK + [R.E_CRC, CR.E_COLOR], st
    sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
    assert (got[N_OK:] == sentinel).all(), "a failed file's slot was written"


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth", [("rgb", 8), ("rgba", 8), ("rgb", 16), ("rgba", 16)])
def test_resize_color_mixed_batch(api, files, mode, depth, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    for dtype in DTYPES:
        kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
        fill = 7 if dtype == "uint" else -3.0
        for filt in ("bilinear", "nearest"):
            st, t, infos = api.png_decode_batch_tensor(datas, RESIZE_TO, mode=mode, depth=depth, dtype=dtype, layout=layout, fill=fill,
                                                       filter=filt, color=Ms, **kw)
            d = api.png_tensor_desc(RESIZE_TO, mode, depth, dtype, layout, **kw)[0]
            got = _np(t)
            assert got.shape == ((6, ch) + RESIZE_TO if layout == "chw" else (6,) + RESIZE_TO + (ch,))
            _check_failed(st, got, fill, dtype)
            plain = None
            if mode == "rgba":  # alpha equals the un-mixed call's alpha plane exactly
                plain = _np(api.png_decode_batch_tensor(datas[:N_OK], RESIZE_TO, mode=mode, depth=depth, dtype=dtype, layout=layout,
                                                        filter=filt, **kw)[1])
            for i in range(N_OK):
                rst, px, inf = _pixels(api, datas[i], mode, depth)
                assert rst == 0 and infos[i] == inf
                want = CR.resize(px, RESIZE_TO, Ms[i], filt, dtype, True, None, list(d.scale), list(d.bias), layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (i, inf, mode, depth, dtype, layout, filt, np.argwhere(got[i] != want)[:4])
                if plain is not None:
                    a_got, a_plain = (got[i][3], plain[i][3]) if layout == "chw" else (got[i][:, :, 3], plain[i][:, :, 3])
                    assert a_got.tobytes() == a_plain.tobytes()


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode,depth", [("rgb", 8), ("rgba", 8), ("rgb", 16), ("rgba", 16)])
def test_warp_color_mixed_batch(api, files, mode, depth, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * ((1 << depth) - 1))) for x in bval] + [0] * (4 - ch)
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=1.7 + 0.2 * k, translate=(1.5 * k, -2.0)) for k, (_, wh) in enumerate(files)]
    flip = [api.png_warp_matrix(wh, WARP_TO, hflip=True, scale=(67 / wh[0], 70 / wh[1])) for _, wh in files]
    q = lambda m: WR.quantise([v for r in m for v in r])  # noqa: E731
    for ws, bmode, filt, dtypes in ((rot, "constant", "bilinear", DTYPES), (flip, "clamp", "bilinear", ["uint", "bfloat16"]),
                                    (rot, "constant", "nearest", ["float32"]), (flip, "clamp", "nearest", ["uint"])):
        for dtype in dtypes:
            kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
            fill = 7 if dtype == "uint" else -3.0
            st, t, infos = api.png_decode_batch_tensor(datas, WARP_TO, mode=mode, depth=depth, dtype=dtype, layout=layout, fill=fill,
                                                       filter=filt, warp=ws, border=bmode,
                                                       border_value=bval if bmode == "constant" else None, color=Ms, **kw)
            d = api.png_tensor_desc(WARP_TO, mode, depth, dtype, layout, antialias=False, **kw)[0]
            got = _np(t)
            _check_failed(st, got, fill, dtype)
            for i in range(N_OK):
                rst, px, inf = _pixels(api, datas[i], mode, depth)
                assert rst == 0 and infos[i] == inf
                want = CR.warp(px, WARP_TO, q(ws[i]), Ms[i], WR.NEAREST if filt == "nearest" else WR.BILINEAR, dtype,
                               WR.CLAMP if bmode == "clamp" else WR.CONSTANT, border, None, list(d.scale), list(d.bias), layout)
                assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
                    (i, inf, mode, depth, dtype, layout, filt, bmode, np.argwhere(got[i] != want)[:4])


def test_exact_consequences_on_the_device(api, files):
    """identity == the call without `color`; hue=120 == that call with its channels rolled; the negative under NEAREST == M - plain;
    for the resize and for the warp"""
    datas = [d for d, _ in files[:N_OK]]
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=2.0) for _, wh in files[:N_OK]]
    for size, wkw in ((RESIZE_TO, {}), (WARP_TO, dict(warp=rot, border="clamp"))):
        for mode, depth in (("rgb", 8), ("rgba", 16)):
            ch = CH[mode]
            top = (1 << depth) - 1
            base = dict(mode=mode, depth=depth, layout="hwc", **wkw)
            for dtype in ("uint", "float32"):
                kw = dict(mean=[0.5] * ch, std=[0.25] * ch) if dtype != "uint" else {}  # (one pair for every channel: a roll keeps it)
                for filt in ("bilinear", "nearest"):
                    call = lambda **k: _np(api.png_decode_batch_tensor(datas, size, dtype=dtype, filter=filt, **base, **kw, **k)[1])  # noqa: E731
                    plain = call()
                    assert call(color=api.png_color_matrix()).tobytes() == plain.tobytes(), (size, mode, dtype, filt, "identity")
                    rolled = plain.copy()
                    rolled[..., :3] = np.roll(plain[..., :3], 1, axis=-1)
                    assert call(color=api.png_color_matrix(hue=120)).tobytes() == rolled.tobytes(), (size, mode, dtype, filt, "hue=120")
                    if dtype == "uint" and filt == "nearest":
                        neg = call(color=CR.NEGATIVE)
                        assert np.array_equal(neg[..., :3], top - plain[..., :3]) and np.array_equal(neg[..., 3:], plain[..., 3:])


def test_one_matrix_for_the_batch_and_the_status_order(api, files):
    datas = [d for d, _ in files]
    M = api.png_color_matrix(contrast=1.5)
    st, t, _ = api.png_decode_batch_tensor(datas, RESIZE_TO, mode="rgb", dtype="uint", layout="hwc", color=M, fill=9)
    assert st == [0] * N_OK + [R.E_CRC, 0]
    got = _np(t)
    assert (got[4] == 9).all()
    for i in (0, 3, 5):
        want = CR.resize(_pixels(api, datas[i], "rgb", 8)[1], RESIZE_TO, M, "bilinear", "uint")
        assert np.array_equal(got[i], want), i
    # E_BOX > E_WARP > E_COLOR > a damaged CRC
    nanw = ((1.0, 0.0, math.nan), (0.0, 1.0, 0.0))
    Ms = np.stack([_matrices(api)[5]] * 4)
    crc = datas[4]
    st, t, _ = api.png_decode_batch_tensor([crc] * 4, (5, 6), mode="rgb", dtype="uint", boxes=[(0, 0, 99, 1), None, None, None],
                                           warp=[nanw, nanw, None, None], color=Ms, fill=3)
    assert st == [Z.E_BOX, WR.E_WARP, CR.E_COLOR, CR.E_COLOR] and (_np(t) == 3).all()
