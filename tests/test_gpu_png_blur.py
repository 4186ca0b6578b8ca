"""Gaussian blur and sharpness on the MI355X (include/decode_png.h: debig_png_decode_batch_tensor_blur;
api.png_decode_batch_tensor(..., blur=)): the whole call BIT FOR BIT against the numpy restatement tests/png_blur_ref.py applied to
the 8-bit result of the existing restatements of the stages in front (png_filter_ref / png_alpha_ref for the resize, png_warp_ref
for the warp, png_color_ref for the matrix, png_tone_ref for the tone table).  One batch of eight small files -- RGB8 70 x 37
(gaussian 23 / 2.0), RGBA8 70 x 37 (gaussian 63 / 10.0), a 4-bit palette file with tRNS 19 x 9 (gaussian 3 / 0.1), grey 8 33 x 21
(sharpness 0.3), RGB8 (sharpness 1.9), RGB8 with no operation, one with a damaged CRC and one with an even ksize --, resized to
19 x 67 and warped to 70 x 67 (partial tiles on both axes; on 19 rows radius 31 folds more than once); alone, after a colour matrix
and after `tone` (equalize and posterize; one file with a tone and no blur operation, one with a blur and no tone operation);
bilinear and bicubic, alpha OVER, modes rgb, rgba and gray, every dtype, both layouts.  The slot of the file without an operation
equals what the call without `blur` writes; the slot of a failed file still holds `fill`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as AR  # noqa: E402
import png_blur_ref as B  # noqa: E402
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
BLURS = [("gaussian", 23, 2.0), ("gaussian", 63, 10.0), ("gaussian", 3, 0.1), ("sharpness", 0.3), ("sharpness", 1.9), None,
         ("gaussian", 23, 2.0), ("gaussian", 4, 1.0)]
OPS = [(B.GAUSSIAN, 23, 2.0), (B.GAUSSIAN, 63, 10.0), (B.GAUSSIAN, 3, 0.1), (B.SHARPNESS, 0, 0.3), (B.SHARPNESS, 0, 1.9), None]
# (file 2 has a blur and no tone operation, file 5 a tone and no blur operation)
TONES = ["equalize", ("posterize", 3), None, "equalize", ("posterize", 2), "equalize", None, None]
TONE_OPS = [(T.EQUALIZE, 0), (T.POSTERIZE, 3), None, (T.EQUALIZE, 0), (T.POSTERIZE, 2), (T.EQUALIZE, 0)]
BACKGROUND = [0.25, 1.0, 0.5]


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A_

    return A_


@pytest.fixture(scope="module")
def files():
    """[(data, (w, h))] in the order of BLURS; file 6 has a damaged CRC"""
    rng = np.random.default_rng(2032)
    ft = lambda p, y: y % 5  # noqa: E731
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(13)]
    trns = bytes(int(v) for v in rng.integers(0, 256, 9))
    specs = [(70, 37, 2, 8, None, None), (70, 37, 6, 8, None, None), (19, 9, 3, 4, pal, trns), (33, 21, 0, 8, None, None),
             (40, 30, 2, 8, None, None), (16, 9, 2, 8, None, None), (16, 9, 2, 8, None, None), (9, 16, 2, 8, None, None)]
    out = []
    for w, h, ct, depth, p, t in specs:
        s = R.random_image(rng, w, h, ct, depth, len(p) if p else None)
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


_PX, _S8, _V = {}, {}, {}


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


def _check(api, files, got, st, infos, d, dtype, layout, fill, mode, tag, how_of, plain, toned):
    """every slot of one call: the blur files against the restatement (computed once per configuration, converted per dtype), the
    file without a blur operation against the call without `blur`, the failed files against `fill`"""
    assert st == [0] * N_OK + [R.E_CRC, B.E_BLUR], st
    sentinel = Z.bf16_bits(np.float32(fill)) if dtype == "bfloat16" else np.array(fill).astype(got.dtype)
    assert (got[N_OK:] == sentinel).all(), "a failed file's slot was written"
    assert got[I_NONE].tobytes() == plain[I_NONE].tobytes(), (tag, "the slot of the file without a blur operation")
    for i in range(N_OK):
        key = (i, mode) + tag
        s8, inf = _stage8(api, key, files[i][0], mode, how_of(i))
        assert infos[i] == inf
        if i == I_NONE:  # (compared with the call without `blur` above)
            continue
        if (key, toned) not in _V:
            if toned and TONE_OPS[i] is not None:
                s8 = T.tone(s8, TONE_OPS[i][0], TONE_OPS[i][1])
            _V[(key, toned)] = B.blur_int(s8, *OPS[i])
        want = Z.convert(_V[(key, toned)], 8, dtype, list(d.scale), list(d.bias))
        if layout == "chw":
            want = np.ascontiguousarray(np.transpose(want, (2, 0, 1)))
        assert got[i].dtype == want.dtype and got[i].tobytes() == want.tobytes(), \
            (i, inf, mode, dtype, layout, tag, toned, np.argwhere(got[i] != want)[:4])
    if dtype == "uint":  # the operations did something (gaussian 3 / 0.1 is the identity)
        assert all(got[i].tobytes() != plain[i].tobytes() for i in (0, 1, 3, 4)), tag
        assert got[2].tobytes() == plain[2].tobytes()


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode", ["rgb", "rgba", "gray"])
def test_resize_blur_mixed_batch(api, files, mode, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    # (filter, alpha, colour matrix, tone, dtypes)
    configs = [("bilinear", "straight", False, False, DTYPES), ("bicubic", "straight", False, False, ["uint", "float32"]),
               ("bilinear", "straight", False, True, DTYPES), ("bicubic", "straight", False, True, ["float16"])]
    if mode != "gray":
        configs += [("bilinear", "straight", True, False, ["uint", "float32"]), ("bilinear", "straight", True, True, ["bfloat16"])]
    if mode != "rgba":
        configs += [("bilinear", "over", False, False, ["uint", "bfloat16"]), ("bicubic", "over", False, True, ["float16"])]
    for filt, alpha, colour, toned, dtypes in configs:
        for dtype in dtypes:
            kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
            if alpha == "over":
                kw.update(alpha="over", background=BACKGROUND[:ch])
            if colour:
                kw.update(color=Ms)
            if toned:
                kw.update(tone=TONES)
            fill = 7 if dtype == "uint" else -3.0
            base = dict(mode=mode, dtype=dtype, layout=layout, fill=fill, filter=filt, **kw)
            st, t, infos = api.png_decode_batch_tensor(datas, RESIZE_TO, blur=BLURS, **base)
            plain = _np(api.png_decode_batch_tensor(datas, RESIZE_TO, **base)[1])
            d = api.png_tensor_desc(RESIZE_TO, mode, 8, dtype, layout, kw.get("mean"), kw.get("std"))[0]
            got = _np(t)
            assert got.shape == ((N, ch) + RESIZE_TO if layout == "chw" else (N,) + RESIZE_TO + (ch,))
            _check(api, files, got, st, infos, d, dtype, layout, fill, mode, ("resize", filt, alpha, colour),
                   lambda i: ("resize", filt, alpha, Ms[i] if colour else None), plain, toned)


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("mode", ["rgb", "rgba", "gray"])
def test_warp_blur_mixed_batch(api, files, mode, layout):
    datas = [d for d, _ in files]
    ch, Ms = CH[mode], _matrices(api)
    bval = [1.0, 0.25, 0.0, 0.5][:ch]
    border = [int(round(x * 255)) for x in bval] + [0] * (4 - ch)
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=1.7 + 0.2 * k, translate=(1.5 * k, -2.0)) for k, (_, wh) in enumerate(files)]
    flip = [api.png_warp_matrix(wh, WARP_TO, hflip=True, scale=(67 / wh[0], 70 / wh[1])) for _, wh in files]
    q = lambda m: WR.quantise([v for r in m for v in r])  # noqa: E731
    # (name, matrices, border, colour matrix, tone, dtypes)
    configs = [("rot", rot, "constant", False, False, DTYPES), ("flip", flip, "clamp", False, False, ["uint"]),
               ("rot", rot, "constant", False, True, ["uint", "float32"])]
    if mode != "gray":
        configs += [("rot", rot, "constant", True, False, ["float32"]), ("rot", rot, "constant", True, True, ["uint", "bfloat16"])]
    for name, ws, bmode, colour, toned, dtypes in configs:
        for dtype in dtypes:
            kw = dict(mean=MEAN[:ch], std=STD[:ch]) if dtype != "uint" else {}
            if colour:
                kw.update(color=Ms)
            if toned:
                kw.update(tone=TONES)
            fill = 7 if dtype == "uint" else -3.0
            base = dict(mode=mode, dtype=dtype, layout=layout, fill=fill, warp=ws, border=bmode,
                        border_value=bval if bmode == "constant" else None, **kw)
            st, t, infos = api.png_decode_batch_tensor(datas, WARP_TO, blur=BLURS, **base)
            plain = _np(api.png_decode_batch_tensor(datas, WARP_TO, **base)[1])
            d = api.png_tensor_desc(WARP_TO, mode, 8, dtype, layout, kw.get("mean"), kw.get("std"), False)[0]
            _check(api, files, _np(t), st, infos, d, dtype, layout, fill, mode, ("warp", name, colour),
                   lambda i: ("warp", q(ws[i]), WR.CLAMP if bmode == "clamp" else WR.CONSTANT, border, Ms[i] if colour else None),
                   plain, toned)


def test_no_operation_for_any_file_is_the_call_without_blur(api, files):
    datas = [d for d, _ in files]
    rot = [api.png_warp_matrix(wh, WARP_TO, angle=30.0, scale=2.0) for _, wh in files]
    M = api.png_color_matrix(1.1, 0.9, 1.2, 10.0)
    tones = ["equalize", None, ("posterize", 3), None, "autocontrast", None, None, ("solarize", 99)]
    for size, kw in ((RESIZE_TO, dict(filter="bicubic", alpha="over", background=BACKGROUND)), (RESIZE_TO, dict(color=M, filter="nearest")),
                     (WARP_TO, dict(warp=rot, border="clamp")), (WARP_TO, dict(warp=rot, color=M, tone=tones)), (RESIZE_TO, {}),
                     (RESIZE_TO, dict(tone=tones))):
        for dtype in DTYPES:
            for layout in ("chw", "hwc"):
                base = dict(mode="rgb", dtype=dtype, layout=layout, fill=5, **kw)
                st0, t0, inf0 = api.png_decode_batch_tensor(datas, size, **base)
                st1, t1, inf1 = api.png_decode_batch_tensor(datas, size, blur=[None] * N, **base)
                assert st0 == st1 == [0] * 6 + [R.E_CRC, 0] and inf0 == inf1
                assert _np(t0).tobytes() == _np(t1).tobytes(), (size, kw.keys(), dtype, layout)


def test_blur_status_order(api, files):
    datas = [d for d, _ in files]
    crc = datas[6]
    import math

    nanw = ((1.0, 0.0, math.nan), (0.0, 1.0, 0.0))
    nanm = np.array(CR.IDENTITY)
    nanm[1, 2] = math.nan
    ident = np.array(CR.IDENTITY)
    Ms = np.stack([nanm, nanm, nanm, ident, ident, ident])
    # E_BOX > E_WARP > E_COLOR > E_TONE > E_BLUR > a damaged CRC
    st, t, _ = api.png_decode_batch_tensor([crc] * 6, (5, 6), mode="rgb", dtype="uint", boxes=[(0, 0, 99, 1)] + [None] * 5,
                                           warp=[nanw, nanw, None, None, None, None], color=Ms, fill=3,
                                           tone=[("solarize", 257)] * 4 + ["equalize"] * 2,
                                           blur=[("gaussian", 3, 0.0)] * 5 + [("sharpness", 16.0)])
    assert st == [Z.E_BOX, WR.E_WARP, CR.E_COLOR, T.E_TONE, B.E_BLUR, R.E_CRC] and (_np(t) == 3).all()
    # every remaining condition, and the limits that are still inside
    st, t, _ = api.png_decode_batch_tensor([datas[5]] * 8, (5, 6), mode="rgb", dtype="uint", fill=3,
                                           blur=[("gaussian", 65, 1.0), ("gaussian", 1, 1.0), ("gaussian", 3, 1000.5), ("gaussian", 3, math.nan),
                                                 ("sharpness", -16.5), ("sharpness", math.inf), ("gaussian", 63, 1000.0), ("sharpness", -16.0)])
    assert st == [B.E_BLUR] * 6 + [0, 0] and (_np(t)[:6] == 3).all()
