"""Gaussian blur and sharpness of the tensor decode (include/decode_png.h: debig_png_decode_batch_tensor_blur), everything that
needs no GPU:
  * debig_png_blur_weights, the C host helper: symmetric, not negative, the sum 16384, every tap within 1 of the restatement's own
    double computation (libm's and numpy's exp may differ in the last place) and equal to it on the parameters the GPU test uses;
    bad ksize / sigma return 0;
  * the restatement tests/png_blur_ref.py against Pillow: SMOOTH bit for bit (L, RGB, RGBA with alpha kept), sharpness within 1 of
    ImageEnhance.Sharpness and exactly equal at factors 0 and 1;
  * the Gaussian restatement against a float64 scipy.ndimage.correlate1d(mode="mirror"): at most 0.05 of an 8-bit step apart in
    real value (0.0233 measured on this list on noise, 0.0406 with the 0 / 255 block channel used here), the uint8 within 1 --
    tests of the rule, not of the kernel;
  * the whole call's argument checks and the rank of E_BLUR among the statuses decided at IHDR; the python wrapper's own checks.
The three tests against Pillow and scipy (test_smooth_is_pillows, test_sharpness_is_within_one_of_pillows,
test_gaussian_against_a_float64_mirrored_convolution) run tests/png_blur_ref.py only, no project code: they show that the rule
which the other tests hold the library and the kernel to is the one Pillow and a float64 convolution mean."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_blur_ref as B  # noqa: E402
import png_color_ref as CR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_tone_ref as T  # noqa: E402
import png_warp_ref as WR  # noqa: E402

BAD_ARG, BAD_FORMAT = -2, -1
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
SENTINEL = 0xABCD
BILINEAR, BICUBIC, NEAREST = 0, 1, 2
STRAIGHT, PREMULTIPLIED, OVER = 0, 1, 2
RGBA, RGB, GRAY, GRAY_ALPHA, D16 = 0, 1, 2, 3, 0x10
IDENT = [v for r in CR.IDENTITY for v in r]
WIDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
PARAMS = [(3, 0.1), (3, 0.8), (5, 1.0), (9, 2.0), (23, 0.1), (23, 2.0), (23, 3.7), (63, 2.0), (63, 10.0), (63, 30.0)]
SIZES = [(37, 70), (19, 67), (9, 5), (96, 96)]  # (H, W)


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_blur_weights.restype = C.c_int
    L.debig_png_blur_weights.argtypes = [C.c_uint32, C.c_double, C.c_void_p]
    L.debig_png_decode_batch_tensor_blur.restype = C.c_int
    L.debig_png_decode_batch_tensor_blur.argtypes = [C.c_void_p] * 8 + [C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint32] + \
        [C.c_void_p] * 4
    return L


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


# ---- the C host helper -----------------------------------------------------------------------------------------------------------

def _host_weights(lib, ksize, sigma):
    q = np.full(63, 0x5A5A, np.int16)
    ok = lib.debig_png_blur_weights(ksize, sigma, q.ctypes.data)
    if not ok:
        return None
    assert not q[ksize:].any()  # zeros behind the taps
    return [int(v) for v in q[:ksize]]


def test_host_weights_are_symmetric_and_sum_to_one(lib, api):
    rng = np.random.default_rng(5)
    cases = PARAMS + [(3, 1000.0), (63, 1000.0), (63, 1e-3)]
    cases += [(int(2 * rng.integers(1, 32) + 1), float(10 ** rng.uniform(-1.5, 2.5))) for _ in range(500)]
    for ksize, sigma in cases:
        q = _host_weights(lib, ksize, sigma)
        assert q is not None and len(q) == ksize, (ksize, sigma)
        assert q == q[::-1] and min(q) >= 0 and sum(q) == 16384, (ksize, sigma, q)
        w = B.weights_real(ksize, sigma) * 16384
        ref = B.weights(ksize, sigma)
        assert sum(ref) == 16384 and ref == ref[::-1]
        # within 1 of the double computation: floor(w + 1/2) is within 1/2 of w, an exp in another last place moves a tap by at
        # most one; the centre tap takes the deficit, so it moves by no more than the other taps together
        moved = 0
        for j, (a, b) in enumerate(zip(q, ref)):
            if j != ksize // 2:
                assert abs(a - b) <= 1 and abs(a - w[j]) <= 1, (ksize, sigma, j)
                moved += abs(a - b)
        assert abs(q[ksize // 2] - ref[ksize // 2]) <= max(moved, 1), (ksize, sigma)
    for ksize, sigma in PARAMS:  # (the device tests compare bit for bit against the restatement's taps)
        assert _host_weights(lib, ksize, sigma) == B.weights(ksize, sigma), (ksize, sigma)
        assert np.array_equal(api.png_blur_weights(ksize, sigma), B.weights(ksize, sigma))
    assert B.weights(3, 0.1) == [0, 16384, 0]


def test_bad_ksize_and_sigma_return_zero(lib, api):
    bad = [(0, 1.0), (1, 1.0), (2, 1.0), (4, 1.0), (62, 1.0), (64, 1.0), (65, 1.0), (0xFFFFFFFF, 1.0), (3, 0.0), (3, -1.0), (3, -0.0),
           (3, 1000.5), (3, math.inf), (3, -math.inf), (3, math.nan), (63, 1e300)]
    for ksize, sigma in bad:
        assert _host_weights(lib, ksize, sigma) is None, (ksize, sigma)
        assert B.weights(ksize, sigma) is None and not B.param_ok(B.GAUSSIAN, ksize, sigma)
    assert api.png_blur_weights(4, 1.0) is None and api.png_blur_weights(3, math.nan) is None and api.png_blur_weights(-3, 1.0) is None
    for factor in (16.0, -16.0, 0.0, 1.9):
        assert B.param_ok(B.SHARPNESS, 0, factor) and B.param_ok(B.SHARPNESS, 77, factor)
    for factor in (16.0001, -17.0, math.inf, math.nan):
        assert not B.param_ok(B.SHARPNESS, 0, factor)
    assert not B.param_ok(3, 3, 1.0)


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------------

def _images(ch):
    rng = np.random.default_rng(70 + ch)
    out = []
    for H, W in SIZES + [(3, 5), (3, 3), (2, 7), (7, 1)]:
        out.append(rng.integers(0, 256, (H, W, ch), dtype=np.uint8))
        blocky = np.repeat(np.repeat(rng.integers(0, 2, (-(-H // 3), -(-W // 3), ch), dtype=np.uint8) * 255, 3, 0), 3, 1)[:H, :W]
        out.append(np.ascontiguousarray(blocky))
    return out


def _pil(img):
    Image = pytest.importorskip("PIL.Image")
    ch = img.shape[2]
    return Image.fromarray(np.ascontiguousarray(img[:, :, 0]) if ch == 1 else img)  # (L, RGB or RGBA by the shape)


def _arr(im, ch):
    a = np.asarray(im)
    return a[:, :, None] if ch == 1 else a


def test_smooth_is_pillows():
    pytest.importorskip("PIL")
    from PIL import ImageFilter

    for ch in (1, 3, 4):
        for img in _images(ch):
            cc = B.colour_channels(ch)
            want = _arr(_pil(img).filter(ImageFilter.SMOOTH), ch)
            got = B.smooth(img)
            assert np.array_equal(got[:, :, :cc], want[:, :, :cc]), (ch, img.shape)
            # factor 0 through the whole rule: SMOOTH on the colour channels, alpha kept
            u8 = B.blur(img, B.SHARPNESS, 0, 0.0)
            assert np.array_equal(u8[:, :, :cc], want[:, :, :cc]) and np.array_equal(u8[:, :, cc:], img[:, :, cc:])


def test_sharpness_is_within_one_of_pillows():
    pytest.importorskip("PIL")
    from PIL import ImageEnhance

    for ch in (1, 3, 4):
        cc = B.colour_channels(ch)
        for img in _images(ch):
            for factor in (0.0, 0.1, 0.5, 1.0, 1.5, 1.9):
                want = _arr(ImageEnhance.Sharpness(_pil(img)).enhance(factor), ch).astype(np.int64)
                got = B.blur(img, B.SHARPNESS, 0, factor).astype(np.int64)
                assert np.array_equal(got[:, :, cc:], img[:, :, cc:]), "alpha passes through"
                d = np.abs(got[:, :, :cc] - want[:, :, :cc])
                assert d.max() <= 1, (ch, img.shape, factor, int(d.max()))
                if factor in (0.0, 1.0):
                    assert d.max() == 0, (ch, img.shape, factor)
            assert np.array_equal(B.blur(img, B.SHARPNESS, 0, 1.0), img)  # factor 1: the identity, alpha included


# ---- the Gaussian restatement against a float64 convolution -----------------------------------------------------------------

def test_gaussian_against_a_float64_mirrored_convolution():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(9)
    worst = 0.0
    for H, W in SIZES:
        noise = rng.integers(0, 256, (H, W, 2), dtype=np.uint8)
        noise[:, :, 1] = np.repeat(np.repeat(rng.integers(0, 2, (-(-H // 4), -(-W // 4)), dtype=np.uint8) * 255, 4, 0), 4, 1)[:H, :W]
        for ksize, sigma in PARAMS:
            w = B.weights_real(ksize, sigma)
            f = noise.astype(np.float64)
            # (scipy's "mirror" needs no more than one reflection: pad by folding first, then convolve without a border)
            r = ksize // 2
            f = f[B.fold(np.arange(-r, H + r), H)][:, B.fold(np.arange(-r, W + r), W)]
            f = ndi.correlate1d(ndi.correlate1d(f, w, axis=1, mode="mirror"), w, axis=0, mode="mirror")[r:r + H, r:r + W]
            if r < min(H, W):  # where scipy's own border rule is defined it is this one
                g = ndi.correlate1d(ndi.correlate1d(noise.astype(np.float64), w, axis=1, mode="mirror"), w, axis=0, mode="mirror")
                assert np.abs(g - f).max() < 1e-9
            v = B.gaussian_int(noise, ksize, sigma)
            err = np.abs(v / float(1 << 22) - f).max()
            print(f"{H}x{W} ksize {ksize} sigma {sigma}: {err:.4f} LSB")
            worst = max(worst, err)
            assert err <= 0.05, (H, W, ksize, sigma, err)
            u8 = B.blur(noise, B.GAUSSIAN, ksize, sigma).astype(np.int64)
            assert np.abs(u8 - np.floor(f + 0.5).astype(np.int64)).max() <= 1, (H, W, ksize, sigma)
    print(f"worst {worst:.4f} LSB")


# ---- the whole call: what needs no device ----------------------------------------------------------------------------------------

class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


def _tdesc(api, fmt=RGB, dtype=0, flags=0, w=8, h=6, layout=0):
    d = api.PngTensorDesc(out_w=w, out_h=h, out_format=fmt, out_layout=layout, dtype=dtype, resize_flags=flags)
    d.scale[:] = [1.0] * 4
    return d


def _wdesc(api, filter=BILINEAR, border_mode=0, alpha_mode=0):
    return api.PngWarpDesc(filter=filter, border_mode=border_mode, alpha_mode=alpha_mode, reserved=0)


def _call(lib, api, files, desc, blurs="none", tones=None, tables=None, n_tables=0, ad=None, fd=None, wd=None, colors=None, warps=None,
          boxes=None, out=DUMMY):
    """blurs: "none", None (a NULL pointer) or [(op, ksize, value)]; tones: None (a NULL pointer) or [(op, param)]"""
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    cs = api._png_colors(np.asarray(colors, np.float64).reshape(n, 3, 4), n) if colors is not None else None
    ws = None
    if warps is not None:
        ws = (api.PngWarp * n)()
        for i, m in enumerate(warps):
            ws[i].m[:] = list(m)
    ts = (api.PngTone * n)(*[api.PngTone(*t) for t in tones]) if tones is not None else None
    bs = None
    if blurs is not None:
        bs = (api.PngBlur * n)(*[api.PngBlur(*b) for b in ([(0, 0, 0.0)] * n if isinstance(blurs, str) else blurs)])
    tb = np.ascontiguousarray(tables, np.uint8) if tables is not None else None
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = lib.debig_png_decode_batch_tensor_blur(ins, sizes, out, bx, ws, cs, ts, tb.ctypes.data if tb is not None else None, n_tables,
                                                bs, st, None, n, 0, ref(desc), ref(ad), ref(fd), ref(wd))
    return rc, list(st)


def test_blur_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    FD, AD = api.PngFilterDesc, api.PngAlphaDesc
    untouched = (BAD_ARG, [SENTINEL])
    none = [(0, 0)]
    # the blur call's own
    assert _call(lib, api, f, _tdesc(api), blurs=None) == untouched
    assert _call(lib, api, f, _tdesc(api), blurs=None, tones=none) == untouched
    for fmt in (RGB | D16, RGBA | D16, GRAY | D16, GRAY_ALPHA | D16):
        assert _call(lib, api, f, _tdesc(api, fmt=fmt)) == untouched, fmt
    assert _call(lib, api, f, _tdesc(api, fmt=RGBA), ad=AD(mode=PREMULTIPLIED)) == untouched
    assert _call(lib, api, f, _tdesc(api), tones=none, tables=None, n_tables=1) == untouched
    # those of the extended calls, unchanged
    for desc, kw in ((None, {}), (_tdesc(api, w=0), {}), (_tdesc(api, dtype=4), {}), (_tdesc(api, flags=2), {}),
                     (_tdesc(api), dict(ad=AD(mode=3))), (_tdesc(api, fmt=RGBA), dict(ad=AD(mode=OVER))),
                     (_tdesc(api), dict(fd=FD(filter=3))), (_tdesc(api), dict(fd=FD(filter=NEAREST, reserved=1))),
                     (_tdesc(api), dict(colors=[IDENT], fd=FD(filter=BICUBIC))), (_tdesc(api, fmt=GRAY), dict(colors=[IDENT])),
                     (_tdesc(api), dict(colors=[IDENT], ad=AD(mode=OVER))), (_tdesc(api), dict(warps=[WIDENT])),
                     (_tdesc(api), dict(wd=_wdesc(api))), (_tdesc(api), dict(warps=[WIDENT], wd=_wdesc(api, filter=BICUBIC))),
                     (_tdesc(api), dict(warps=[WIDENT], wd=_wdesc(api), fd=FD(filter=NEAREST)))):
        assert _call(lib, api, f, desc, **kw) == untouched, (desc, kw)
    assert _call(lib, api, f, _tdesc(api), out=DUMMY + 8) == untouched
    assert _call(lib, api, f, _tdesc(api, fmt=4), blurs=None) == (BAD_FORMAT, [SENTINEL])  # the extended call's check comes first
    assert lib.debig_png_decode_batch_tensor_blur(None, None, None, None, None, None, None, None, 0, None, None, None, 0, 0, None, None,
                                                  None, None) == 0
    # accepted, with and without tones: the file is looked at
    g, s = (B.GAUSSIAN, 23, 2.0), (B.SHARPNESS, 0, 0.3)
    for desc, kw in ((_tdesc(api), {}), (_tdesc(api), dict(blurs=[g])),
                     (_tdesc(api, fmt=GRAY, flags=1), dict(ad=AD(mode=OVER), fd=FD(filter=BICUBIC), blurs=[s])),
                     (_tdesc(api, fmt=RGBA, dtype=1, layout=1), dict(ad=AD(mode=STRAIGHT), tones=[(T.EQUALIZE, 0)], blurs=[g])),
                     (_tdesc(api, fmt=GRAY_ALPHA, dtype=3), dict(tones=none, blurs=[s])),
                     (_tdesc(api), dict(colors=[IDENT], fd=FD(filter=NEAREST), blurs=[g])),
                     (_tdesc(api, fmt=RGBA, dtype=2), dict(warps=[WIDENT], wd=_wdesc(api), colors=[IDENT], tones=[(T.POSTERIZE, 3)], blurs=[s]))):
        assert _call(lib, api, f, desc, **kw) == (0, [R.E_SIGNATURE]), (desc, kw)


def test_blur_status_is_decided_on_the_host_behind_box_warp_color_and_tone(lib, api):
    """E_BOX, then E_WARP, then E_COLOR, then E_TONE, then E_BLUR, as soon as IHDR has been read: each outranks what the file holds
    later; the walk's own statuses before the end of IHDR come first"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    crc = bytearray(rgb)
    crc[-20] ^= 1
    crc = bytes(crc)
    nanm = list(IDENT)
    nanm[7] = math.nan
    wnan = (1.0, 0.0, math.nan, 0.0, 1.0, 0.0)
    Bx, Wp, Cl, Tn, Bl = Z.E_BOX, WR.E_WARP, CR.E_COLOR, T.E_TONE, B.E_BLUR
    assert Bl == 19 and api.PNG_STATUS[Bl] == "blur"
    # every E_BLUR condition once, on files whose later fault (a damaged CRC, a missing IDAT) it outranks
    conds = [(B.GAUSSIAN, 4, 1.0), (B.GAUSSIAN, 1, 1.0), (B.GAUSSIAN, 65, 1.0), (B.GAUSSIAN, 0, 1.0), (B.GAUSSIAN, 3, 0.0),
             (B.GAUSSIAN, 3, -2.0), (B.GAUSSIAN, 3, 1000.5), (B.GAUSSIAN, 3, math.nan), (B.GAUSSIAN, 3, math.inf),
             (B.SHARPNESS, 0, 16.5), (B.SHARPNESS, 0, -16.5), (B.SHARPNESS, 0, math.nan), (B.SHARPNESS, 3, -math.inf), (3, 3, 1.0),
             (0xFFFFFFFF, 3, 1.0)]
    for c in conds:
        assert not B.param_ok(*c)
    assert _call(lib, api, [crc if k & 1 else rgb[:40] for k in range(len(conds))], _tdesc(api), blurs=conds) == (0, [Bl] * len(conds))
    files = [rgb, crc, rgb[:40], crc, crc, rgb[:30], b"\x89PNG"]
    boxes = [(0, 0, 10, 1), None, None, None, None, None, None]
    bad = [(B.GAUSSIAN, 4, 1.0)] * 7
    tones = [(T.POSTERIZE, 9)] * 4 + [(T.NONE, 0)] * 3
    colors = [nanm, nanm, nanm, IDENT, IDENT, nanm, nanm]
    warps = [wnan, wnan, WIDENT, WIDENT, WIDENT, wnan, wnan]
    want = [Bx, Wp, Cl, Tn, Bl, R.E_CHUNK, R.E_SIGNATURE]
    assert _call(lib, api, files, _tdesc(api), blurs=bad, tones=tones, boxes=boxes, colors=colors, warps=warps, wd=_wdesc(api)) == (0, want)
    want = [Bx, Cl, Cl, Tn, Bl, R.E_CHUNK, R.E_SIGNATURE]
    assert _call(lib, api, files, _tdesc(api), blurs=bad, tones=tones, boxes=boxes, colors=colors) == (0, want)
    want = [Bx, Tn, Tn, Tn, Bl, R.E_CHUNK, R.E_SIGNATURE]
    assert _call(lib, api, files, _tdesc(api, fmt=GRAY, dtype=1, flags=1), blurs=bad, tones=tones, boxes=boxes,
                 ad=api.PngAlphaDesc(mode=OVER), fd=api.PngFilterDesc(filter=BICUBIC)) == (0, want)
    want = [Bx, Bl, Bl, Bl, Bl, R.E_CHUNK, R.E_SIGNATURE]  # tones NULL
    assert _call(lib, api, files, _tdesc(api), blurs=bad, boxes=boxes) == (0, want)
    # a valid operation leaves the later status (files that fail on the host only: no device is reached); NONE ignores its fields
    ok = [(B.GAUSSIAN, 63, 1000.0), (B.SHARPNESS, 99, -16.0), (B.NONE, 4, math.nan)]
    st = _call(lib, api, [rgb[:40], rgb[:30], b"\x89PNG"], _tdesc(api), blurs=ok)
    assert st[0] == 0 and st[1][1:] == [R.E_CHUNK, R.E_SIGNATURE] and st[1][0] not in (0, Bl, SENTINEL)


# ---- the python wrapper ------------------------------------------------------------------------------------------------------------

def test_python_argument_checks(api):
    """raised before the library or a device is touched"""
    for kw in (dict(depth=16), dict(alpha="premultiplied", mode="rgba")):
        with pytest.raises(ValueError):
            api.png_decode_batch_tensor([b""], (4, 4), blur=[("sharpness", 0.5)], **kw)
    for bad in ([("sharpness", 0.5), None], ["gaussian"], ["sharpness"], [3], [1.5], [{"gaussian": 3}], [("gaussian", 3)], [("sharpness", 1, 2)], [("blur", 3, 1.0)],
                [("gaussian", 3, 1.0, 1.0)], [()], [("none",)]):
        with pytest.raises(ValueError):
            api._png_blurs(bad, 1)
    bs = api._png_blurs([None, ("gaussian", 23, 2.0), ("sharpness", 1.9), ("gaussian", 4, 0.0), ("gaussian", -3, 1.0), ("gaussian", 3.5, 1.0),
                         ("sharpness", -2)], 7)
    assert [(b.op, b.ksize, b.value) for b in bs] == [(0, 0, 0.0), (1, 23, 2.0), (2, 0, 1.9), (1, 4, 0.0), (1, 0, 1.0), (1, 0, 1.0),
                                                      (2, 0, -2.0)]
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["blur"].default is None and list(sig)[-1] == "filter" and list(sig)[-2] == "blur"  # (`filter` stays the last parameter)
