"""The tone curves of the tensor decode (include/decode_png.h: debig_png_decode_batch_tensor_tone), everything that needs no GPU:
  * the numpy restatement tests/png_tone_ref.py against Pillow's ImageOps -- equalize, posterize and solarize bit for bit,
    autocontrast equal wherever (i - lo) * 255 is no multiple of hi - lo and at most 1 apart elsewhere, for all 32,640 (lo, hi);
  * debig_png_tone_table, the C host helper, bit for bit against the restatement on 2,000 random histograms and the edge cases;
  * every E_TONE condition; the whole call's argument checks and the rank of E_TONE among the statuses decided at IHDR;
  * the python wrapper's own checks and the de-duplication of the caller's tables."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageOps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------------

def _equalize_images():
    rng = np.random.default_rng(7)
    out = []
    for h, w in ((3, 5), (16, 16), (20, 20), (19, 67), (70, 67)):  # step 0 (identity); step 1, entries above 255; larger
        out.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    one = rng.integers(0, 256, (19, 67, 3), dtype=np.uint8)
    one[..., 1] = 93  # a channel of one value
    out.append(one)
    out.append((rng.integers(0, 2, (70, 67, 3), dtype=np.uint8) * 201 + 7).astype(np.uint8))  # two values
    out.append((rng.integers(0, 256, (70, 67, 3), dtype=np.uint8) // 32 * 32).astype(np.uint8))  # quantised noise
    out.append((rng.integers(0, 256, (70, 67, 3)).astype(np.float64) ** 2 / 256).astype(np.uint8))  # skewed
    return out


def test_equalize_is_pillows():
    clamped = 0
    for img in _equalize_images():
        for arr, mode in ((img, "RGB"), (img[..., 0], "L")):
            want = np.asarray(ImageOps.equalize(Image.fromarray(arr, mode)))
            a3 = arr if arr.ndim == 3 else arr[..., None]
            got = T.tone(a3, T.EQUALIZE, 0)
            assert np.array_equal(got.reshape(want.shape), want), (img.shape, mode)
        h = T.histogram(img, 1)[0]
        nzi = np.nonzero(h)[0]
        step = (int(h.sum()) - int(h[nzi[-1]])) // 255
        if img.shape[:2] == (3, 5):
            assert step == 0 and T.table(T.EQUALIZE, 0, h) == T.IDENTITY
        if step == 1:
            clamped += int(h.sum()) // step > 255  # (the unclamped last entries pass 255)
    assert clamped >= 2  # 16 x 16 and 20 x 20
    assert T.table(T.EQUALIZE, 0, [0] * 256) == T.IDENTITY and T.table(T.EQUALIZE, 0, [0] * 9 + [5] + [0] * 246) == T.IDENTITY


def test_posterize_and_solarize_are_pillows():
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    im = Image.fromarray(ramp, "L")
    for bits in range(1, 9):
        assert np.array_equal(np.asarray(ImageOps.posterize(im, bits)).reshape(-1), T.table(T.POSTERIZE, bits)), bits
    for thr in range(0, 257):
        assert np.array_equal(np.asarray(ImageOps.solarize(im, thr)).reshape(-1), T.table(T.SOLARIZE, thr)), thr
    assert T.table(T.POSTERIZE, 8) == T.IDENTITY and T.table(T.SOLARIZE, 256) == T.IDENTITY
    assert T.table(T.SOLARIZE, 0) == [255 - i for i in range(256)]


def test_autocontrast_against_pillows_double_rule():
    """all 32,640 pairs: equal wherever (i - lo) * 255 mod (hi - lo) != 0, at most 1 apart elsewhere; lo -> 0 and hi -> 255"""
    pairs = differing = 0
    for lo in range(256):
        for hi in range(lo + 1, 256):
            h = [0] * 256
            h[lo] = 3
            h[hi] = 1
            ours = np.array(T.table(T.AUTOCONTRAST, 0, h), np.int64)
            pil = np.array(T.pillow_autocontrast_table(lo, hi), np.int64)
            i = np.arange(256)
            exact = ((i - lo) * 255) % (hi - lo) == 0
            assert np.array_equal(ours[~exact], pil[~exact]), (lo, hi)
            assert np.abs(ours - pil).max() <= 1, (lo, hi)
            assert ours[lo] == 0 and ours[hi] == 255 and (ours[:lo] == 0).all() and (ours[hi:] == 255).all(), (lo, hi)
            differing += int((ours != pil).sum())
            pairs += 1
    assert pairs == 32640
    print("autocontrast entries that differ from Pillow's double rule:", differing, "of", pairs * 256)
    # the double rule above is what the installed Pillow does: a sample of pairs through ImageOps.autocontrast itself
    rng = np.random.default_rng(3)
    for lo, hi in [(0, 25), (0, 255), (7, 8), (100, 101)] + [tuple(sorted(rng.choice(256, 2, replace=False))) for _ in range(60)]:
        ramp = np.arange(256, dtype=np.uint8)
        lo, hi = int(lo), int(hi)
        img = np.clip(ramp, lo, hi).astype(np.uint8)
        got = np.asarray(ImageOps.autocontrast(Image.fromarray(img.reshape(16, 16), "L"))).reshape(-1)
        assert np.array_equal(got, np.array(T.pillow_autocontrast_table(lo, hi), np.uint8)[img]), (lo, hi)
    assert T.pillow_autocontrast_table(0, 25)[25] == 254 and T.table(T.AUTOCONTRAST, 0, [1] * 26 + [0] * 230)[25] == 255
    assert T.table(T.AUTOCONTRAST, 0, [0] * 256) == T.IDENTITY and T.table(T.AUTOCONTRAST, 0, [0] * 200 + [9] + [0] * 55) == T.IDENTITY


# ---- the C host helper -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_tone_table.restype = C.c_int
    L.debig_png_tone_table.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.debig_png_decode_batch_tensor_tone.restype = C.c_int
    L.debig_png_decode_batch_tensor_tone.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + \
        [C.c_void_p] * 4
    return L


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


def _host_table(lib, op, param, hist):
    h = np.ascontiguousarray(hist, np.uint32) if hist is not None else None
    lut = np.full(256, 0x5A, np.uint8)
    ok = lib.debig_png_tone_table(op, param, h.ctypes.data if h is not None else None, lut.ctypes.data)
    return [int(v) for v in lut] if ok else None


def test_host_helper_equals_the_restatement(lib, api):
    rng = np.random.default_rng(11)
    hists = [np.zeros(256, np.uint32)]
    one = np.zeros(256, np.uint32)
    one[77] = 1 << 28
    two = np.zeros(256, np.uint32)
    two[[0, 255]] = (1 << 28, 5)
    near = np.zeros(256, np.uint32)
    near[[10, 11]] = (254, 3)  # S = 254: step 0
    full = np.full(256, 1 << 28, np.uint32)  # 2^36 in all: sums need 64 bits
    big = np.full(256, 0xFFFFFFFF, np.uint32)
    hists += [one, two, near, full, big]
    while len(hists) < 2000:
        k = len(hists)
        h = rng.integers(0, 1 << int(rng.integers(1, 29)), 256).astype(np.uint32)
        if k % 3 == 0:  # sparse: few occupied bins
            h[rng.random(256) < rng.uniform(0.5, 0.99)] = 0
        if k % 7 == 0:
            h[int(rng.integers(0, 256))] = 1 << 28
        if k % 11 == 0:  # a narrow occupied range
            lo = int(rng.integers(0, 250))
            h[:lo] = 0
            h[lo + int(rng.integers(1, 6)):] = 0
        hists.append(h)
    for k, h in enumerate(hists):
        for op in (T.AUTOCONTRAST, T.EQUALIZE):
            assert _host_table(lib, op, 0, h) == T.table(op, 0, h), (k, op)
    for bits in range(1, 9):
        assert _host_table(lib, T.POSTERIZE, bits, None) == T.table(T.POSTERIZE, bits) == _host_table(lib, T.POSTERIZE, bits, hists[7])
    for thr in range(0, 257):
        assert _host_table(lib, T.SOLARIZE, thr, None) == T.table(T.SOLARIZE, thr)
    assert np.array_equal(api.png_tone_table("equalize", 0, hists[9]), T.table(T.EQUALIZE, 0, hists[9]))
    assert np.array_equal(api.png_tone_table("posterize", 3), T.table(T.POSTERIZE, 3))
    assert api.png_tone_table("posterize", 9) is None and api.png_tone_table(6, 0, hists[9]) is None


def test_every_tone_condition_returns_zero(lib):
    h = np.ones(256, np.uint32)
    bad = [(6, 0), (7, 0), (0xFFFFFFFF, 0), (T.AUTOCONTRAST, 1), (T.EQUALIZE, 1), (T.EQUALIZE, 0xFFFFFFFF), (T.POSTERIZE, 0),
           (T.POSTERIZE, 9), (T.POSTERIZE, 0xFFFFFFFF), (T.SOLARIZE, 257), (T.SOLARIZE, 0xFFFFFFFF),
           (T.TABLE, 0), (T.NONE, 0), (T.NONE, 1)]  # (TABLE and NONE have no table of their own)
    for op, param in bad:
        assert _host_table(lib, op, param, h) is None, (op, param)
        if op not in (T.TABLE, T.NONE):
            assert T.table(op, param, h) is None, (op, param)
    assert not T.param_ok(T.TABLE, 2, 2) and T.param_ok(T.TABLE, 1, 2) and not T.param_ok(T.NONE, 1)
    assert _host_table(lib, T.EQUALIZE, 0, None) is None  # a histogram operation without a histogram


# ---- the whole call: what needs no device ----------------------------------------------------------------------------------------

class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


def _tdesc(api, fmt=RGB, dtype=0, flags=0, w=8, h=6, layout=0):
    d = api.PngTensorDesc(out_w=w, out_h=h, out_format=fmt, out_layout=layout, dtype=dtype, resize_flags=flags)
    d.scale[:] = [1.0] * 4
    return d


def _wdesc(api, filter=BILINEAR, border_mode=0, border=(0, 0, 0, 0), alpha_mode=0, reserved=0):
    d = api.PngWarpDesc(filter=filter, border_mode=border_mode, alpha_mode=alpha_mode, reserved=reserved)
    d.border[:] = list(border)
    return d


def _adesc(api, mode, reserved=0):
    return api.PngAlphaDesc(mode=mode, reserved=reserved)


def _call(lib, api, files, desc, tones="none", tables=None, n_tables=0, ad=None, fd=None, wd=None, colors=None, warps=None, boxes=None,
          out=DUMMY):
    """tones: "none", None (a NULL pointer) or [(op, param)]; colors / warps: None or one flat list per file"""
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
    ts = None
    if tones is not None:
        ts = (api.PngTone * n)(*[api.PngTone(*t) for t in ([(0, 0)] * n if isinstance(tones, str) else tones)])
    tb = np.ascontiguousarray(tables, np.uint8) if tables is not None else None
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    rc = lib.debig_png_decode_batch_tensor_tone(ins, sizes, out, bx, ws, cs, ts, tb.ctypes.data if tb is not None else None, n_tables,
                                                st, None, n, 0, ref(desc), ref(ad), ref(fd), ref(wd))
    return rc, list(st)


def test_tone_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    FD = api.PngFilterDesc
    untouched = (BAD_ARG, [SENTINEL])
    # the tone call's own
    assert _call(lib, api, f, _tdesc(api), tones=None) == untouched
    for fmt in (RGB | D16, RGBA | D16, GRAY | D16, GRAY_ALPHA | D16):
        assert _call(lib, api, f, _tdesc(api, fmt=fmt)) == untouched, fmt
    assert _call(lib, api, f, _tdesc(api, fmt=RGBA), ad=_adesc(api, PREMULTIPLIED)) == untouched
    assert _call(lib, api, f, _tdesc(api, fmt=GRAY_ALPHA), ad=_adesc(api, PREMULTIPLIED)) == untouched
    assert _call(lib, api, f, _tdesc(api), tables=None, n_tables=1) == untouched
    # those of the extended calls, unchanged: the tensor call's, alpha's, the filter's
    for desc, kw in ((None, {}), (_tdesc(api, w=0), {}), (_tdesc(api, dtype=4), {}), (_tdesc(api, flags=2), {}),
                     (_tdesc(api), dict(ad=_adesc(api, 3))), (_tdesc(api), dict(ad=_adesc(api, OVER, reserved=1))),
                     (_tdesc(api, fmt=RGBA), dict(ad=_adesc(api, OVER))), (_tdesc(api), dict(ad=_adesc(api, PREMULTIPLIED))),
                     (_tdesc(api), dict(fd=FD(filter=3))), (_tdesc(api), dict(fd=FD(filter=NEAREST, reserved=1)))):
        assert _call(lib, api, f, desc, **kw) == untouched, (desc, kw)
    assert _call(lib, api, f, _tdesc(api), out=DUMMY + 8) == untouched
    assert _call(lib, api, f, _tdesc(api, fmt=4)) == (BAD_FORMAT, [SENTINEL])  # the extended call's check comes first
    assert _call(lib, api, f, _tdesc(api, fmt=4), tones=None) == (BAD_FORMAT, [SENTINEL])
    # the colour call's
    ci = [IDENT]
    for desc, kw in ((_tdesc(api), dict(fd=FD(filter=BICUBIC))), (_tdesc(api, fmt=GRAY), {}), (_tdesc(api, fmt=GRAY_ALPHA), {}),
                     (_tdesc(api), dict(ad=_adesc(api, STRAIGHT))), (_tdesc(api), dict(ad=_adesc(api, OVER)))):
        assert _call(lib, api, f, desc, colors=ci, **kw) == untouched, (desc, kw)
    # the warp calls'
    wi = [WIDENT]
    for desc, kw in ((_tdesc(api), dict(wd=_wdesc(api, filter=BICUBIC))), (_tdesc(api), dict(wd=_wdesc(api, alpha_mode=OVER))),
                     (_tdesc(api), dict(wd=_wdesc(api, border_mode=2))), (_tdesc(api, flags=1), dict(wd=_wdesc(api))),
                     (_tdesc(api), dict(wd=_wdesc(api, border=(0, 256, 0, 0)))), (_tdesc(api), dict(wd=None)),
                     (_tdesc(api), dict(wd=_wdesc(api), fd=FD(filter=NEAREST))), (_tdesc(api), dict(wd=_wdesc(api), ad=_adesc(api, STRAIGHT))),
                     (_tdesc(api, fmt=GRAY), dict(wd=_wdesc(api), colors=ci))):
        assert _call(lib, api, f, desc, warps=wi, **kw) == untouched, (desc, kw)
    assert _call(lib, api, f, _tdesc(api), wd=_wdesc(api)) == untouched  # a warp descriptor without warps
    assert lib.debig_png_decode_batch_tensor_tone(None, None, None, None, None, None, None, None, 0, None, None, 0, 0, None, None, None,
                                                  None) == 0
    # accepted: the file is looked at
    tab = np.arange(256, dtype=np.uint8)
    for desc, kw in ((_tdesc(api), {}), (_tdesc(api, fmt=GRAY, flags=1), dict(ad=_adesc(api, OVER), fd=FD(filter=BICUBIC))),
                     (_tdesc(api, fmt=RGBA, dtype=1, layout=1), dict(ad=_adesc(api, STRAIGHT), tones=[(T.EQUALIZE, 0)])),
                     (_tdesc(api, fmt=GRAY_ALPHA, dtype=3), dict(tones=[(T.TABLE, 0)], tables=tab, n_tables=1)),
                     (_tdesc(api), dict(colors=ci, fd=FD(filter=NEAREST), tones=[(T.SOLARIZE, 256)])),
                     (_tdesc(api, fmt=GRAY), dict(warps=wi, wd=_wdesc(api, filter=NEAREST, border_mode=1), tones=[(T.POSTERIZE, 1)])),
                     (_tdesc(api, fmt=RGBA, dtype=2), dict(warps=wi, wd=_wdesc(api), colors=ci, tones=[(T.AUTOCONTRAST, 0)]))):
        assert _call(lib, api, f, desc, **kw) == (0, [R.E_SIGNATURE]), (desc, kw)


def test_tone_status_is_decided_on_the_host_behind_box_warp_and_color(lib, api):
    """E_BOX, then E_WARP, then E_COLOR, then E_TONE, as soon as IHDR has been read: each outranks what the file holds later (a
    damaged CRC, a missing IDAT); the walk's own statuses before the end of IHDR come first"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    crc = bytearray(rgb)
    crc[-20] ^= 1
    crc = bytes(crc)
    nanm = list(IDENT)
    nanm[7] = math.nan
    wnan = (1.0, 0.0, math.nan, 0.0, 1.0, 0.0)
    B, Wp, Cl, Tn = Z.E_BOX, WR.E_WARP, CR.E_COLOR, T.E_TONE
    assert Tn == 18 and api.PNG_STATUS[Tn] == "tone"
    files = [rgb, crc, rgb[:40], rgb, rgb[:30], b"\x89PNG", crc, crc]
    boxes = [(0, 0, 10, 1), None, None, None, None, None, None, None]
    tab = np.zeros((2, 256), np.uint8)
    # every E_TONE condition once
    tones = [(T.POSTERIZE, 9), (6, 0), (T.EQUALIZE, 1), (T.SOLARIZE, 257), (T.POSTERIZE, 0), (T.TABLE, 2), (T.TABLE, 2), (T.NONE, 1)]
    want = [B, Tn, Tn, Tn, R.E_CHUNK, R.E_SIGNATURE, Tn, Tn]
    assert _call(lib, api, files, _tdesc(api), tones=tones, tables=tab, n_tables=2, boxes=boxes) == (0, want)
    assert _call(lib, api, files, _tdesc(api, fmt=GRAY, dtype=1, flags=1), tones=tones, tables=tab, n_tables=2, boxes=boxes,
                 ad=_adesc(api, OVER), fd=api.PngFilterDesc(filter=BICUBIC)) == (0, want)
    # a valid tone leaves the later status: the damaged CRC is found on the device, so only files that fail on the host are used
    ok = [(T.EQUALIZE, 0), (T.TABLE, 1), (T.SOLARIZE, 0)]
    st = _call(lib, api, [rgb[:40], rgb[:30], b"\x89PNG"], _tdesc(api), tones=ok, tables=tab, n_tables=2)
    assert st[0] == 0 and st[1][1:] == [R.E_CHUNK, R.E_SIGNATURE] and st[1][0] not in (0, Tn, SENTINEL)
    # with a colour matrix and a warp: E_BOX > E_WARP > E_COLOR > E_TONE > later statuses
    colors = [nanm, nanm, nanm, IDENT, nanm, nanm, IDENT, nanm]
    warps = [wnan, wnan, WIDENT, WIDENT, wnan, wnan, WIDENT, WIDENT]
    want = [B, Wp, Cl, Tn, R.E_CHUNK, R.E_SIGNATURE, Tn, Cl]
    assert _call(lib, api, files, _tdesc(api), tones=tones, tables=tab, n_tables=2, boxes=boxes, colors=colors, warps=warps,
                 wd=_wdesc(api)) == (0, want)
    want = [B, Cl, Cl, Tn, R.E_CHUNK, R.E_SIGNATURE, Tn, Cl]
    assert _call(lib, api, files, _tdesc(api), tones=tones, tables=tab, n_tables=2, boxes=boxes, colors=colors) == (0, want)


# ---- the python wrapper ------------------------------------------------------------------------------------------------------------

def test_python_argument_checks_and_table_deduplication(api):
    """raised before the library or a device is touched"""
    for kw in (dict(depth=16), dict(alpha="premultiplied", mode="rgba")):
        with pytest.raises(ValueError):
            api.png_decode_batch_tensor([b""], (4, 4), tone=["equalize"], **kw)
    for bad in (["equalize", None], ["sharpen"], ["posterize"], [("table", np.zeros(255, np.uint8))], [("table", np.full(256, 256))],
                [("equalize", 0, 0)], ["none"]):
        with pytest.raises(ValueError):
            api._png_tones(bad, 1)
    g1 = np.arange(256, dtype=np.uint8)[::-1].copy()
    g2 = (np.arange(256) // 2).astype(np.uint8)
    ts, tabs, n = api._png_tones([None, "autocontrast", "equalize", ("posterize", 3), ("solarize", 100), ("table", g1), ("table", g2),
                                  ("table", list(g1)), ("posterize", 9), ("solarize", -1)], 10)
    assert [(t.op, t.param) for t in ts] == [(0, 0), (1, 0), (2, 0), (3, 3), (4, 100), (5, 0), (5, 1), (5, 0), (3, 9), (4, 0xFFFFFFFF)]
    assert n == 2 and tabs.tobytes() == g1.tobytes() + g2.tobytes()
    assert api._png_tones([None, None], 2)[1:] == (None, 0)
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["tone"].default is None and list(sig)[-1] == "filter"  # (`filter` stays the last parameter)
