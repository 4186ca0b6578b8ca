"""Tone curves on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_tone; api.png_decode_batch_tensor(..., tone=)): the
whole call BIT FOR BIT against the numpy restatement tests/png_tone_ref.py applied to the 8-bit result of the existing restatements
of the first stage (png_filter_ref / png_alpha_ref for the resize, png_warp_ref for the warp, png_color_ref for the matrix).  One
batch of eight small files -- RGB8 70 x 37 (equalize), RGBA8 70 x 37 (autocontrast), a 4-bit palette file with tRNS 19 x 9
(solarize 100), grey 8 33 x 21 (posterize 3), RGB8 (a gamma table), RGB8 with no operation, one with a damaged CRC and one with
("posterize", 9) --, resized to 19 x 67 and warped to 70 x 67 (4690 pixels: two pixel runs per file); with and without a colour
matrix, bilinear and bicubic, alpha OVER, modes rgb, rgba and gray, every dtype, both layouts.  The slot of the file without an
operation equals what the call without `tone` writes; the slot of a failed file still holds `fill`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as AR  # noqa: E402
import png_color_ref as CR  # noqa: E402
import png_filter_ref as FR  # noqa: E402
import png_out_format_ref as F  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_tone_ref as T  # noqa: E402
import png_warp_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
RESIZE_TO, WARP_TO = (19, 67), (70, 67)  # (H, W)
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
CH = {"rgba": 4, "rgb": 3, "gray": 1}
WITH_ALPHA = {"rgb": "rgba", "gray": "gray_alpha"}
DTYPES = ["uint", "float32", "float16", "bfloat16"]
N, N_OK, I_NONE = 8, 6, 5
GAMMA = np.array([min(255, int(255.0 * (i / 255.0) ** 0.5 + 0.5)) for i in range(256)], np.uint8)
TONES = ["equalize", "autocontrast", ("solarize", 100), ("posterize", 3), ("table", GAMMA), None, "equalize", ("posterize", 9)]
OPS = [(T.EQUALIZE, 0), (T.AUTOCONTRAST, 0), (T.SOLARIZE, 100), (T.POSTERIZE, 3), (T.TABLE, 0), (T.NONE, 0)]
BACKGROUND = [0.25, 1.0, 0.5]


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def files():
    """[(data, (w, h))] in the order of TONES; file 6 has a damaged CRC"""
    rng = np.random.default_rng(2031)
    ft = lambda p, y: y % 5  # noqa: E731
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(13)]
    trns = bytes(int(v) for v in rng.integers(0, 256, 9))
    specs = [(70, 37, 2, 8, None, None), (70, 37, 6, 8, None, None), (19, 9, 3, 4, pal, trns), (33, 21, 0, 8, None, None),
             (40, 30, 2, 8, None, None), (16, 9, 2, 8, None, None), (16, 9, 2, 8, None, None), (9, 16, 2, 8, None, None)]
    out = []
    for k, (w, h, ct, depth, p, t) in enumerate(specs):
        s = R.random_image(rng, w, h, ct, depth, len(p) if p else None)
        if k == 0:  # a narrow, skewed range: the equalize and autocontrast tables are far from the identity
            s = (np.asarray(s).astype(np.uint32) ** 2 // 400 + 30).astype(np.asarray(s).dtype)
        out.append((R.encode(s, ct, depth, 0, trns=t, palette=p, filters=ft), (w, h)))
    b = bytearray(out[6][0])
    b[-20] ^= 1  # inside the last IDAT's payload: its CRC no longer matches
    out[6] = (bytes(b), out[6][1])
    return out


def _matrices(api):
    """one per file, all different"""
    return np.stack([api.png_color_matrix(1.2, 0.8, 1.3, 17.0), api.png_color_matrix(0.7, 1.4, 0.2, -60.0),
                     np.array([[2.0, -1.5, 0.7, -0.1], [-0.6, 1.9, -0.4, 0.3], [0.2, 0.4, -2.0, 1.1]]),
                     api.png_color_matrix(saturation=0.0), api.png_color_matrix(0.5, 0.6), api.png_color_matrix(hue=120),
                     api.png_color_matrix(), api.png_color_matrix()])


def _np(t):
    import torch

    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


_PX, _S8 = {}, {}


def _pixels(api, data, mode):
    """the restatement's decode of a file in a tensor format of depth 8, computed once"""
    if (data, mode) not in _PX:
        _PX[(data, mode)] = F.decode(data, api.png_out_format(mode, 8))
    return _PX[(data, mode)]


def _stage8(api, key, data, mode, how):
    """the 8-bit HWC result of the first stage for one file, computed once per configuration.  how: ("resize", filter, alpha, M)
    or ("warp", m, border mode, border, M)"""
    if key not in _S8:
        if how[0] == "resize":
            _, filt, alpha, M = how
            if alpha == "over":
                rst, px, inf = _pixels(api, data, WITH_ALPHA[mode])
                bg = AR.background_samples(BACKGROUND[:CH[mode]], CH[mode], 8)
                s8 = FR.resize(px, RESIZE_TO, filt, "uint", True, alpha="over", background=bg)
            else:
                rst, px, inf = _pixels(api, data, mode)
                s8 = CR.resize(px, RESIZE_TO, M, filt, "uint") if M is not None else FR.resize(px, RESIZE_TO, filt, "uint")
        else:
            _, m, bmode, border, M = how
            rst, px, inf = _pixels(api, data, mode)
            s8 = CR.warp(px, WARP_TO, m, M, WR.BILINEAR, "uint", bmode, border)
        assert rst == 0 and s8.dtype == np.uint8
        _S8[key] = (s8, inf)
    return _S8[key]


def _check(api, files, got, st, infos, d, dtype, layout, fill, mode, tag, how_of, plain):
    """every slot of one call: the tone files against the restatement, the file without an operation against the call without
    `tone`, the failed files against `fill`"""
    assert st == [0] * N_OK + [R.E_CRC, T.E_TONE], st
    sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
    assert (got[N_OK:] == sentinel).all(), "a failed file's slot was written"
    assert got[I_NONE].tobytes() == plain[I_NONE].tobytes(), (tag, "the slot of the file without an operation")
    for i in range(N_OK):
        s8, inf = _stage8(api, (i, mode) + tag, files[i][0], mode, how_of(i))
        assert infos[i] == inf
        if i == I_NONE:  # (it does not go through the 8-bit intermediate: compared with the call without `tone` above)
            continue
        op, param = OPS[i]
        want = T.tone(s8, op, param, dtype, list(d.scale), list(d.bias), layout, GAMMA)
        assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
            (i, inf, mode, dtype, layout, tag, np.argwhere(got[i] != want)[:4])
    if dtype == "uint":  # the operations did something (autocontrast may be the identity: a full-range image stays as it is)
        assert all(got[i].tobytes() != plain[i].tobytes() for i in (0, 2, 3, 4)), tag


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode", ["rgb", "rgba", "gray"])
def test_resize_tone_mixed_batch(api, files, mode, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    configs = [("bilinear", "straight", False, DTYPES), ("bicubic", "straight", False, ["uint", "float32"])]
    if mode != "gray":
        configs.append(("bilinear", "straight", True, DTYPES))
    if mode != "rgba":
        configs += [("bilinear", "over", False, ["uint", "bfloat16"]), ("bicubic", "over", False, ["float16"])]
    for filt, alpha, colour, dtypes in configs:
        for dtype in dtypes:
            kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
            if alpha == "over":
                kw.update(alpha="over", background=BACKGROUND[:ch])
            if colour:
                kw.update(color=Ms)
            fill = 7 if dtype == "uint" else -3.0
            base = dict(mode=mode, dtype=dtype, layout=layout, fill=fill, filter=filt, **kw)
            st, t, infos = api.png_decode_batch_tensor(datas, RESIZE_TO, tone=TONES, **base)
            plain = _np(api.png_decode_batch_tensor(datas, RESIZE_TO, **base)[1])
            d = api.png_tensor_desc(RESIZE_TO, mode, 8, dtype, layout, kw.get("mean"), kw.get("std"))[0]
            got = _np(t)
            assert got.shape == ((N, ch) + RESIZE_TO if layout == "chw" else (N,) + RESIZE_TO + (ch,))
            _check(api, files, got, st, infos, d, dtype, layout, fill, mode, ("resize", filt, alpha, colour),
                   lambda i: ("resize", filt, alpha, Ms[i] if colour else None), plain)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode", ["rgb", "rgba", "gray"])
def test_warp_tone_mixed_batch(api, files, mode, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * 255)) for x in bval] + [0] * (4 - ch)
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=1.7 + 0.2 * k, translate=(1.5 * k, -2.0)) for k, (_, wh) in enumerate(files)]
    flip = [api.png_warp_matrix(wh, WARP_TO, hflip=True, scale=(67 / wh[0], 70 / wh[1])) for _, wh in files]
    q = lambda m: WR.quantise([v for r in m for v in r])  # noqa: E731
    configs = [("rot", rot, "constant", False, DTYPES), ("flip", flip, "clamp", False, ["uint"])]
    if mode != "gray":
        configs.append(("rot", rot, "constant", True, DTYPES))
    for name, ws, bmode, colour, dtypes in configs:
        for dtype in dtypes:
            kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
            if colour:
                kw.update(color=Ms)
            fill = 7 if dtype == "uint" else -3.0
            base = dict(mode=mode, dtype=dtype, layout=layout, fill=fill, warp=ws, border=bmode,
                        border_value=bval if bmode == "constant" else None, **kw)
            st, t, infos = api.png_decode_batch_tensor(datas, WARP_TO, tone=TONES, **base)
            plain = _np(api.png_decode_batch_tensor(datas, WARP_TO, **base)[1])
            d = api.png_tensor_desc(WARP_TO, mode, 8, dtype, layout, kw.get("mean"), kw.get("std"), False)[0]
            _check(api, files, _np(t), st, infos, d, dtype, layout, fill, mode, ("warp", name, colour),
                   lambda i: ("warp", q(ws[i]), WR.CLAMP if bmode == "clamp" else WR.CONSTANT, border, Ms[i] if colour else None), plain)
    # the rotation leaves the crop somewhere: elements that the CONSTANT border produced were counted in the histograms
    jx, jy = WR.picks(WARP_TO, q(rot[0]))
    assert ((jx < 0) | (jx >= files[0][1][0]) | (jy < 0) | (jy >= files[0][1][1])).any()


def test_no_operation_for_any_file_is_the_call_without_tone(api, files):
    datas = [d for d, _ in files]
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=2.0) for _, wh in files]
    M = api.png_color_matrix(1.1, 0.9, 1.2, 10.0)
    for size, kw in ((RESIZE_TO, dict(filter="bicubic", alpha="over", background=BACKGROUND)), (RESIZE_TO, dict(color=M, filter="nearest")),
                     (WARP_TO, dict(warp=rot, border="clamp")), (WARP_TO, dict(warp=rot, color=M)), (RESIZE_TO, {})):
        for dtype in DTYPES:
            for layout in ("chw", "hwc"):
                base = dict(mode="rgb", dtype=dtype, layout=layout, fill=5, **kw)
                st0, t0, inf0 = api.png_decode_batch_tensor(datas, size, **base)
                st1, t1, inf1 = api.png_decode_batch_tensor(datas, size, tone=[None] * N, **base)
                assert st0 == st1 == [0] * 6 + [R.E_CRC, 0] and inf0 == inf1
                assert _np(t0).tobytes() == _np(t1).tobytes(), (size, kw.keys(), dtype, layout)


def test_tone_status_order_and_shared_tables(api, files):
    datas = [d for d, _ in files]
    crc = datas[6]
    import math

    nanw = ((1.0, 0.0, math.nan), (0.0, 1.0, 0.0))
    nanm = np.array(CR.IDENTITY)
    nanm[1, 2] = math.nan
    Ms = np.stack([nanm, nanm, nanm, np.array(CR.IDENTITY), np.array(CR.IDENTITY)])
    # E_BOX > E_WARP > E_COLOR > E_TONE > a damaged CRC
    st, t, _ = api.png_decode_batch_tensor([crc] * 5, (5, 6), mode="rgb", dtype="uint", boxes=[(0, 0, 99, 1), None, None, None, None],
                                           warp=[nanw, nanw, None, None, None], color=Ms, fill=3,
                                           tone=[("solarize", 257)] * 4 + ["equalize"])
    assert st == [Z.E_BOX, WR.E_WARP, CR.E_COLOR, T.E_TONE, R.E_CRC] and (_np(t) == 3).all()
    # two files share one caller's table, a third has its own; posterize 8 and solarize 256 are the identity
    inv = np.arange(256, dtype=np.uint8)[::-1].copy()
    st, t, _ = api.png_decode_batch_tensor([datas[0]] * 5, RESIZE_TO, mode="rgb", dtype="uint", layout="hwc",
                                           tone=[("table", inv), ("table", GAMMA), ("table", inv), ("posterize", 8), ("solarize", 256)])
    got = _np(t)
    plain = _np(api.png_decode_batch_tensor([datas[0]], RESIZE_TO, mode="rgb", dtype="uint", layout="hwc")[1])[0]
    assert st == [0] * 5
    assert np.array_equal(got[0], 255 - plain) and np.array_equal(got[2], got[0]) and np.array_equal(got[1], GAMMA[plain])
    assert np.array_equal(got[3], plain) and np.array_equal(got[4], plain)
