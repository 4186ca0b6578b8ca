"""The affine warp without a GPU (include/decode_png.h: debig_png_decode_batch_tensor_warp, debig_png_decode_batch_labels_warp):
the host quantiser against the restatement (tests/png_warp_ref.py), what the two C calls decide on the host alone -- the
argument checks (status left at its sentinel) and E_WARP with its place in the order of statuses -- and api.png_warp_matrix:
its closed forms and the order in which its operations compose."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_ref as LR  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402

BAD_ARG, BAD_FORMAT = -2, -1
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
SENTINEL = 0xABCD
BILINEAR, BICUBIC, NEAREST = 0, 1, 2
U8, U16, I32, I64 = range(4)
RGB, RGBA, GRAY, D16 = 1, 0, 2, 0x10
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_warp_quantise.restype = C.c_int
    L.debig_png_warp_quantise.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    for name in ("debig_png_decode_batch_tensor_warp", "debig_png_decode_batch_labels_warp"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


# ---- the quantiser -------------------------------------------------------------------------------------------------------------

def _host_q(lib, M):
    m = (C.c_int64 * 6)(*[SENTINEL] * 6)
    ok = lib.debig_png_warp_quantise((C.c_double * 6)(*M), m)
    return list(m) if ok else None


def test_quantise_random_matrices(lib):
    rng = np.random.default_rng(16)
    for k in range(4000):
        lin = rng.uniform(-1, 1, 4) * 10.0 ** rng.integers(-6, 5)
        tr = rng.uniform(-1, 1, 2) * 10.0 ** rng.integers(-3, 8)
        M = [lin[0], lin[1], tr[0], lin[2], lin[3], tr[1]]
        if k % 7 == 0:  # exact halves of a Q16 unit, both signs: away from zero
            M[k % 6] = (int(rng.integers(-1000, 1000)) + 0.5) / 65536.0
        want = WR.quantise(M)
        assert _host_q(lib, M) == want, M
        if want is not None:
            assert all(abs(a - b * 65536.0) <= 0.5 for a, b in zip(want, M))
    assert _host_q(lib, [0.5 / 65536, -0.5 / 65536, 1.5 / 65536, -1.5 / 65536, 0.49999 / 65536, -0.49999 / 65536]) == [1, -1, 2, -2, 0, 0]
    assert _host_q(lib, [0.49999999999999994 / 65536] * 6) == [0] * 6  # (x + 0.5 would round up in float64)


def test_quantise_limits(lib):
    """the exact limits pass; one step of float64 beyond each limit, NaN and the infinities are E_WARP"""
    top = [32768.0, 32768.0, 2.0 ** 24, 32768.0, 32768.0, 2.0 ** 24]
    for sign in (1.0, -1.0):
        M = [sign * v for v in top]
        want = [int(sign) * (1 << 31), int(sign) * (1 << 31), int(sign) * (1 << 40)] * 2
        assert _host_q(lib, M) == want and WR.quantise(M) == want
        for k in range(6):
            for beyond in (math.nextafter(M[k], sign * math.inf), sign * math.inf, math.nan):
                B = list(IDENT)
                B[k] = beyond
                assert _host_q(lib, B) is None and WR.quantise(B) is None, (k, beyond)
            B = list(IDENT)
            B[k] = math.nextafter(M[k], 0.0)  # one step inside
            assert _host_q(lib, B) == WR.quantise(B) != None  # noqa: E711
    assert _host_q(lib, IDENT) == [65536, 0, 0, 0, 65536, 0]
    assert _host_q(lib, [0.0] * 6) == [0] * 6  # singular matrices are legal
    assert _host_q(lib, [5e-324, -5e-324, 0, 0, 0, 0]) == [0] * 6


# ---- the C calls: what needs no device -------------------------------------------------------------------------------------------

def _files(files, boxes, warps):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    ins._bufs = bufs
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    ws = None
    if warps is not None:
        from debigulator_amd.api import PngWarp

        ws = (PngWarp * n)()
        for i, m in enumerate(warps):
            ws[i].m[:] = list(m)
    return ins, sizes, st, bx, ws


def _tensor_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, warps="ident"):
    ins, sizes, st, bx, ws = _files(files, boxes, [IDENT] * len(files) if warps == "ident" else warps)
    rc = lib.debig_png_decode_batch_tensor_warp(ins, sizes, out, bx, ws, st, None, len(files), 0,
                                                C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None)
    return rc, list(st)


def _label_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, warps="ident"):
    ins, sizes, st, bx, ws = _files(files, boxes, [IDENT] * len(files) if warps == "ident" else warps)
    rc = lib.debig_png_decode_batch_labels_warp(ins, sizes, out, bx, ws, st, None, len(files), 0,
                                                C.byref(desc) if desc is not None else None, C.byref(wd) if wd is not None else None)
    return rc, list(st)


def _tdesc(api, fmt=RGB, dtype=0, flags=0, w=8, h=6, layout=0):
    d = api.PngTensorDesc(out_w=w, out_h=h, out_format=fmt, out_layout=layout, dtype=dtype, resize_flags=flags)
    d.scale[:] = [1.0] * 4
    return d


def _wdesc(api, filter=BILINEAR, border_mode=0, border=(0, 0, 0, 0), alpha_mode=0, reserved=0):
    d = api.PngWarpDesc(filter=filter, border_mode=border_mode, alpha_mode=alpha_mode, reserved=reserved)
    d.border[:] = list(border)
    return d


def test_tensor_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    bad = [
        (_tdesc(api), _wdesc(api, filter=BICUBIC)),                 # bicubic is not provided with a warp
        (_tdesc(api), _wdesc(api, filter=3)),
        (_tdesc(api), _wdesc(api, alpha_mode=1)),                   # premultiplied
        (_tdesc(api), _wdesc(api, alpha_mode=2)),                   # over
        (_tdesc(api), _wdesc(api, border_mode=2)),
        (_tdesc(api), _wdesc(api, reserved=1)),
        (_tdesc(api, flags=1), _wdesc(api)),                        # antialias is not provided under a warp
        (_tdesc(api), _wdesc(api, border=(0, 0, 256, 0))),          # a used channel above 2^8 - 1
        (_tdesc(api, fmt=GRAY), _wdesc(api, border=(256, 0, 0, 0))),
        (_tdesc(api), None),
        (None, _wdesc(api)),
        (_tdesc(api, w=0), _wdesc(api)),                            # the checks of the call that is extended
        (_tdesc(api, dtype=4), _wdesc(api)),
    ]
    for desc, wd in bad:
        assert _tensor_call(lib, api, f, desc, wd) == (BAD_ARG, [SENTINEL]), (desc, wd)
    assert _tensor_call(lib, api, f, _tdesc(api), _wdesc(api), warps=None) == (BAD_ARG, [SENTINEL])
    assert _tensor_call(lib, api, f, _tdesc(api), _wdesc(api), out=DUMMY + 8) == (BAD_ARG, [SENTINEL])
    assert _tensor_call(lib, api, f, _tdesc(api, fmt=4), _wdesc(api)) == (BAD_FORMAT, [SENTINEL])
    assert lib.debig_png_decode_batch_tensor_warp(None, None, None, None, None, None, None, 0, 0, None, None) == 0
    # at the edge of their ranges the arguments pass and the file is reached
    for desc, wd in ((_tdesc(api), _wdesc(api, filter=NEAREST, border_mode=1)),
                     (_tdesc(api), _wdesc(api, border=(255, 255, 255, 256))),          # the fourth channel is not used by RGB
                     (_tdesc(api, fmt=RGBA | D16, dtype=3), _wdesc(api, border=(65535,) * 4)),
                     (_tdesc(api), _wdesc(api, border_mode=1, border=(999, 999, 999, 999)))):  # CLAMP does not read the border
        assert _tensor_call(lib, api, f, desc, wd) == (0, [R.E_SIGNATURE])


def test_label_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    LD, LW = api.PngLabelDesc, api.PngLabelWarpDesc
    bad = [(LD(out_w=8, out_h=6, dtype=U8), LW(0, 256)), (LD(out_w=8, out_h=6, dtype=U8), LW(0, -1)),
           (LD(out_w=8, out_h=6, dtype=U16), LW(0, 65536)), (LD(out_w=8, out_h=6, dtype=U16), LW(0, -1)),
           (LD(out_w=8, out_h=6, dtype=I64), LW(2, 0)), (LD(out_w=8, out_h=6, dtype=I64), None), (None, LW(0, 0)),
           (LD(out_w=0, out_h=6, dtype=I64), LW(0, 0)), (LD(out_w=8, out_h=6, dtype=4), LW(0, 0)),
           (LD(out_w=8, out_h=6, dtype=I32, reserved=1), LW(0, 0))]
    for desc, wd in bad:
        assert _label_call(lib, api, f, desc, wd) == (BAD_ARG, [SENTINEL]), (desc, wd)
    assert _label_call(lib, api, f, LD(out_w=8, out_h=6, dtype=I64), LW(0, 0), warps=None) == (BAD_ARG, [SENTINEL])
    assert lib.debig_png_decode_batch_labels_warp(None, None, None, None, None, None, None, 0, 0, None, None) == 0
    for desc, wd in ((LD(out_w=8, out_h=6, dtype=U8), LW(0, 255)), (LD(out_w=8, out_h=6, dtype=U16), LW(0, 65535)),
                     (LD(out_w=8, out_h=6, dtype=I32), LW(0, -1)), (LD(out_w=8, out_h=6, dtype=I64), LW(0, -2 ** 31)),
                     (LD(out_w=8, out_h=6, dtype=U8), LW(1, -1))):  # CLAMP does not read border_label
        assert _label_call(lib, api, f, desc, wd) == (0, [R.E_SIGNATURE])


def test_warp_status_is_decided_on_the_host_behind_label_and_box(lib, api):
    """E_LABEL, then E_BOX, then E_WARP, as soon as IHDR has been read: each outranks what the file holds later (a damaged CRC,
    a missing IDAT); the walk's own statuses before IHDR come first; one file per pair of neighbours in the order"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    g8 = R.encode(R.random_image(rng, 9, 7, 0, 8), 0, 8)
    g8_crc = bytearray(g8)
    g8_crc[-20] ^= 1
    nan = (1.0, 0.0, math.nan, 0.0, 1.0, 0.0)
    big = (1.0, 32768.5, 0.0, 0.0, 1.0, 0.0)
    far = (1.0, 0.0, 0.0, 0.0, 1.0, -2.0 ** 24 - 4)
    L, B, Wp = LR.E_LABEL, LR.E_BOX, WR.E_WARP
    files = [rgb, rgb, g8, bytes(g8_crc), g8[:40], g8[:30], b"\x89PNG"]
    boxes = [(0, 0, 10, 1), None, (0, 0, 10, 1), None, None, None, None]
    warps = [nan, nan, big, far, nan, big, nan]
    ld = api.PngLabelDesc(out_w=8, out_h=6, dtype=I64)
    # labels: E_LABEL > E_BOX (file 0), E_LABEL > E_WARP (1), E_BOX > E_WARP (2), E_WARP > CRC (3), E_WARP > missing IDAT (4);
    # a walk error before the end of IHDR stands (5, 6)
    assert _label_call(lib, api, files, ld, api.PngLabelWarpDesc(0, -1), boxes=boxes, warps=warps) == \
        (0, [L, L, B, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE])
    # the tensor call has no E_LABEL: the RGB files' box and matrix decide
    assert _tensor_call(lib, api, files, _tdesc(api), _wdesc(api), boxes=boxes, warps=warps) == \
        (0, [B, Wp, B, Wp, Wp, R.E_CHUNK, R.E_SIGNATURE])
    assert api.PNG_STATUS[WR.E_WARP] == "warp"


# ---- png_warp_matrix -------------------------------------------------------------------------------------------------------------

def test_warp_matrix_closed_forms(api):
    """the identity, the flips and the quarter turns are exactly the matrices the header lists"""
    w, h = 13, 7
    mat = api.png_warp_matrix
    assert mat((w, h), (h, w)) == ((1, 0, 0), (0, 1, 0))
    assert mat((w, h), (h, w), hflip=True) == ((-1, 0, w), (0, 1, 0))
    assert mat((w, h), (h, w), vflip=True) == ((1, 0, 0), (0, -1, h))
    assert mat((w, h), (w, h), angle=90) == ((0, -1, w), (1, 0, 0))
    assert mat((w, h), (h, w), angle=180) == ((-1, 0, w), (0, -1, h))
    assert mat((w, h), (w, h), angle=270) == mat((w, h), (w, h), angle=-90) == ((0, 1, 0), (-1, 0, h))
    assert mat((w, h), (h, w), hflip=True, vflip=True) == mat((w, h), (h, w), angle=180)
    assert mat((w, h), (h, w), angle=360) == mat((w, h), (h, w))
    assert not any(math.copysign(1.0, v) < 0 and v == 0 for r in mat((w, h), (h, w), vflip=True) for v in r)  # no negative zeros
    # an enlargement about the centres, a translation in output pixels
    assert mat((4, 4), (8, 8), scale=2) == ((0.5, 0, 0), (0, 0.5, 0))
    assert mat((4, 4), (4, 4), translate=(3, -1)) == ((1, 0, -3), (0, 1, 1))
    for kw in (dict(scale=0), dict(scale=(1, 0)), dict(shear=(45, 45))):
        with pytest.raises(ValueError):
            mat((4, 4), (4, 4), **kw)


def _apply(px, size, M, filt=WR.NEAREST):
    return WR.warp(px, size, WR.quantise([v for r in M for v in r]), filt)


def test_warp_matrix_composition_order(api):
    """flips, then scale, then shear, then the rotation, then the translation -- seen from the source to the output"""
    rng = np.random.default_rng(3)
    w, h = 13, 7
    px = rng.integers(0, 256, size=(h, w, 2)).astype(np.uint8)
    mat = api.png_warp_matrix
    for filt in (WR.NEAREST, WR.BILINEAR):
        # the flip comes before the rotation
        got = _apply(px, (w, h), mat((w, h), (w, h), angle=90, hflip=True), filt)
        assert np.array_equal(got, np.rot90(np.fliplr(px), 1)) and not np.array_equal(got, np.fliplr(np.rot90(px, 1)))
        # the translation comes last, in output pixels: after a quarter turn it still moves the picture right and down
        got = _apply(px, (w, h), mat((w, h), (w, h), angle=90, translate=(2, 1)), filt)
        turned = np.rot90(px, 1)
        assert np.array_equal(got[1:, 2:], turned[:-1, :-2]) and not got[0].any() and not got[:, :2].any()
    # scale before the rotation: an anisotropic scale stretches the SOURCE's x axis, which the turn then stands upright
    got = _apply(px, (2 * w, h), mat((w, h), (2 * w, h), angle=90, scale=(2, 1)))
    assert np.array_equal(got, np.rot90(np.repeat(px, 2, axis=1), 1))
    # shear before the rotation: the general linear part is flips^-1 scale^-1 shear^-1 rotation^-1 of the inverse chain
    M = mat((w, h), (h, w), angle=30, scale=(1.5, 0.5), shear=(10, -5), hflip=True)
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    tx, ty = math.tan(math.radians(10)), math.tan(math.radians(-5))
    fwd = np.array([[c, s], [-s, c]]) @ np.array([[1, tx], [ty, 1]]) @ np.diag([1.5, 0.5]) @ np.diag([-1.0, 1.0])
    lin = np.array([M[0][:2], M[1][:2]])
    assert np.allclose(lin @ fwd, np.eye(2), atol=1e-12)
    centre = lin @ np.array([w / 2, h / 2]) + np.array([M[0][2], M[1][2]])  # the output centre lands on the source centre
    assert np.allclose(centre, [w / 2, h / 2], atol=1e-9)


def test_python_descriptor_checks(api):
    d = api.png_warp_desc("nearest", "clamp")
    assert (d.filter, d.border_mode, d.alpha_mode, d.reserved) == (NEAREST, 1, 0, 0)
    d = api.png_warp_desc(border_value=(1.0, 0.5, 0.0), depth=16)
    assert list(d.border) == [65535, 32768, 0, 0]
    assert list(api.png_warp_desc(border_value=1.0, mode="gray").border) == [255, 0, 0, 0]
    for kw in (dict(filter="bicubic"), dict(alpha="over"), dict(alpha="premultiplied", mode="rgba"), dict(border="wrap"),
               dict(border_value=(1, 1)), dict(border_value=1.5), dict(border="clamp", border_value=0.5), dict(depth="native")):
        with pytest.raises(ValueError):
            api.png_warp_desc(**kw)
    assert (api.png_label_warp_desc().border_mode, api.png_label_warp_desc(border_label=-1).border_label) == (0, -1)
    for kw in (dict(border_label=256, dtype="uint8"), dict(border_label=-1, dtype="uint16"), dict(border="clamp", border_label=3),
               dict(border="mirror"), dict(dtype="float32")):
        with pytest.raises(ValueError):
            api.png_label_warp_desc(**kw)
    with pytest.raises(ValueError):
        api._png_warps([None], 2)
    with pytest.raises(ValueError):
        api._png_warps([(1, 0, 0, 1)], 1)
    ws = api._png_warps([None, ((0, -1, 5), (1, 0, 0))], 2)
    assert list(ws[0].m) == list(IDENT) and list(ws[1].m) == [0, -1, 5, 1, 0, 0]
    # the keywords that belong to a warp are refused without one, before any device is looked for
    for fn, kw in ((api.png_decode_batch_tensor, dict(border="clamp")), (api.png_decode_batch_tensor, dict(border_value=0.5)),
                   (api.png_decode_batch_labels, dict(border="clamp")), (api.png_decode_batch_labels, dict(border_label=255))):
        with pytest.raises(ValueError):
            fn([b""], (4, 4), **kw)
    for kw in (dict(filter="bicubic"), dict(alpha="over")):
        with pytest.raises(ValueError):
            api.png_decode_batch_tensor([b""], (4, 4), warp=[None], **kw)
