"""The per-image colour matrix without a GPU (include/decode_png.h: debig_png_decode_batch_tensor_color,
debig_png_decode_batch_tensor_warp_color): the host quantiser against the restatement (tests/png_color_ref.py), what the two C
calls decide on the host alone -- the argument checks (status left at its sentinel) and E_COLOR with its place in the order of
statuses --, api.png_color_matrix, and the integer mix against float64."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_color_ref as CR  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402
import png_warp_ref as WR  # noqa: E402

BAD_ARG, BAD_FORMAT = -2, -1
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
SENTINEL = 0xABCD
BILINEAR, BICUBIC, NEAREST = 0, 1, 2
RGBA, RGB, GRAY, GRAY_ALPHA, D16 = 0, 1, 2, 3, 0x10
IDENT = [v for r in CR.IDENTITY for v in r]
WIDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_color_quantise.restype = C.c_int
    L.debig_png_color_quantise.argtypes = [C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.debig_png_decode_batch_tensor_color.restype = C.c_int
    L.debig_png_decode_batch_tensor_color.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.debig_png_decode_batch_tensor_warp_color.restype = C.c_int
    L.debig_png_decode_batch_tensor_warp_color.argtypes = [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def api():
    from debigulator_amd import api as A_

    return A_


# ---- the quantiser -------------------------------------------------------------------------------------------------------------

def _host_q(lib, M, P):
    k = (C.c_int32 * 9)(*[-77] * 9)
    o = (C.c_int64 * 3)(*[-77] * 3)
    ok = lib.debig_png_color_quantise((C.c_double * 12)(*[float(v) for v in np.asarray(M, np.float64).reshape(-1)]), P, k, o)
    return (list(k), list(o)) if ok else None


def test_quantise_bounds_and_identity(lib):
    for P in (8, 16):
        assert _host_q(lib, IDENT, P) == CR.quantise(IDENT, P) == ([65536, 0, 0, 0, 65536, 0, 0, 0, 65536], [0, 0, 0])
        for sign in (1.0, -1.0):
            for j in range(12):
                M = list(IDENT)
                M[j] = sign * 16.0  # the limit itself is accepted
                got = _host_q(lib, M, P)
                assert got is not None and got == CR.quantise(M, P)
                if j % 4 == 3:
                    assert got[1][j // 4] == int(sign) * 16 * CR.vmax(P)
                else:
                    assert got[0][3 * (j // 4) + j % 4] == int(sign) * (1 << 20)
                for beyond in (sign * 16.0001, math.nextafter(sign * 16.0, sign * math.inf), sign * math.inf, math.nan):
                    M[j] = beyond
                    assert _host_q(lib, M, P) is None and CR.quantise(M, P) is None, (j, beyond)
    assert _host_q(lib, IDENT, 12) is None  # a precision the tensor calls do not have


def test_quantise_random_matrices(lib):
    rng = np.random.default_rng(17)
    for n in range(2000):
        M = rng.uniform(-1, 1, 12) * 10.0 ** rng.integers(-6, 2)
        if n % 5 == 0:  # exact halves of a Q16 unit, both signs: away from zero
            M[n % 12 // 4 * 4 + n % 3] = (int(rng.integers(-1000, 1000)) + 0.5) / 65536.0
        for P in (8, 16):
            assert _host_q(lib, M, P) == CR.quantise(M, P), (M, P)
    assert _host_q(lib, [0.5 / 65536, -0.5 / 65536, 1.5 / 65536, 0.0] * 3, 8)[0] == [1, -1, 2] * 3
    assert _host_q(lib, [0.0, 0.0, 0.0, 1.0] * 3, 8)[1] == [255 << 22] * 3 and _host_q(lib, [0.0, 0.0, 0.0, -1.0] * 3, 16)[1] == [-(65535 << 14)] * 3


# ---- png_color_matrix ------------------------------------------------------------------------------------------------------------

def test_color_matrix_closed_forms(api):
    mat = api.png_color_matrix
    assert np.array_equal(mat(), np.array(CR.IDENTITY)) and not np.signbit(mat()).any()
    cyc = {120: [0, 0, 65536, 65536, 0, 0, 0, 65536, 0], 240: [0, 65536, 0, 0, 0, 65536, 65536, 0, 0]}
    for hue, k in cyc.items():
        for P in (8, 16):
            assert CR.quantise(mat(hue=hue), P) == (k, [0, 0, 0]), hue
    # hue = 120 takes R to the G output: out = (B, R, G)
    assert np.array_equal(CR.mix_float64(np.array([[0.25, 0.5, 0.75]]), np.round(mat(hue=120))), [[0.75, 0.25, 0.5]])
    luma = (6968 / 32768, 23434 / 32768, 2366 / 32768)
    assert np.array_equal(mat(saturation=0), np.array([luma + (0.0,)] * 3))
    assert np.array_equal(mat(brightness=1.5), 1.5 * np.array(CR.IDENTITY))
    assert np.array_equal(mat(contrast=0.5), np.array([[0.5, 0, 0, 0.25], [0, 0.5, 0, 0.25], [0, 0, 0.5, 0.25]]))
    assert np.array_equal(mat(contrast=2.0, center=0.25)[:, 3], [-0.25] * 3)
    # the order: brightness, then contrast, then saturation, then hue
    x = np.random.default_rng(5).uniform(0, 1, (50, 3))
    b, c, s, h = 1.3, 0.7, 1.6, 40.0
    y = b * x
    y = c * y + (1 - c) * 0.5
    y = s * y + (1 - s) * (y @ np.array(luma))[:, None]
    ch, sh = math.cos(math.radians(h)), math.sin(math.radians(h))
    Hm = ch * np.eye(3) + (1 - ch) / 3 + sh / math.sqrt(3) * np.array([[0, -1, 1], [1, 0, -1], [-1, 1, 0]])
    y = y @ Hm.T
    M = mat(b, c, s, h)
    assert np.allclose(x @ M[:, :3].T + M[:, 3], y, atol=1e-12)
    assert np.allclose(Hm @ np.ones(3), np.ones(3)) and np.allclose(Hm @ Hm.T, np.eye(3))  # a rotation about the grey axis
    with pytest.raises(ValueError):
        mat(luma=(1, 0))


def test_python_argument_checks(api):
    """raised before the library or a device is touched"""
    M = api.png_color_matrix(brightness=1.1)
    for kw in (dict(filter="bicubic"), dict(alpha="over"), dict(alpha="premultiplied", mode="rgba"), dict(mode="gray"),
               dict(mode="gray_alpha"), dict(warp=[None], filter="bicubic")):
        with pytest.raises(ValueError):
            api.png_decode_batch_tensor([b""], (4, 4), color=M, **kw)
    with pytest.raises(ValueError):
        api._png_colors(np.zeros((2, 3, 4)), 3)
    with pytest.raises(ValueError):
        api._png_colors(np.zeros((3, 3)), 1)
    cs = api._png_colors(M, 2)
    assert list(cs[0].m) == list(cs[1].m) == list(M.reshape(-1))
    cs = api._png_colors([CR.IDENTITY, CR.NEGATIVE], 2)
    assert list(cs[1].m) == [v for r in CR.NEGATIVE for v in r]
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["color"].default is None and list(sig)[-1] == "filter"  # (`filter` stays the last parameter)
    assert api.PNG_STATUS[CR.E_COLOR] == "color"


# ---- the C calls: what needs no device -------------------------------------------------------------------------------------------

def _files(api, files, boxes, colors, warps):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    ins._bufs = bufs
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes else None
    cs = api._png_colors(np.asarray(colors, np.float64).reshape(n, 3, 4), n) if colors is not None else None
    ws = None
    if warps is not None:
        ws = (api.PngWarp * n)()
        for i, m in enumerate(warps):
            ws[i].m[:] = list(m)
    return ins, sizes, st, bx, cs, ws


def _color_call(lib, api, files, desc, fd=None, out=DUMMY, boxes=None, colors="ident"):
    ins, sizes, st, bx, cs, _ = _files(api, files, boxes, [IDENT] * len(files) if isinstance(colors, str) else colors, None)
    rc = lib.debig_png_decode_batch_tensor_color(ins, sizes, out, bx, cs, st, None, len(files), 0,
                                                 C.byref(desc) if desc is not None else None, C.byref(fd) if fd is not None else None)
    return rc, list(st)


def _warp_color_call(lib, api, files, desc, wd, out=DUMMY, boxes=None, colors="ident", warps="ident"):
    ins, sizes, st, bx, cs, ws = _files(api, files, boxes, [IDENT] * len(files) if isinstance(colors, str) else colors,
                                        [WIDENT] * len(files) if isinstance(warps, str) else warps)
    rc = lib.debig_png_decode_batch_tensor_warp_color(ins, sizes, out, bx, ws, cs, st, None, len(files), 0,
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


def test_color_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    FD = api.PngFilterDesc
    bad = [(_tdesc(api), FD(filter=BICUBIC)), (_tdesc(api), FD(filter=3)), (_tdesc(api), FD(filter=NEAREST, reserved=1)),
           (_tdesc(api, fmt=GRAY), None), (_tdesc(api, fmt=GRAY_ALPHA | D16), None), (None, None),
           (_tdesc(api, w=0), None), (_tdesc(api, dtype=4), None), (_tdesc(api, flags=2), None)]
    for desc, fd in bad:
        assert _color_call(lib, api, f, desc, fd) == (BAD_ARG, [SENTINEL]), (desc, fd)
    assert _color_call(lib, api, f, _tdesc(api), colors=None) == (BAD_ARG, [SENTINEL])
    assert _color_call(lib, api, f, _tdesc(api), out=DUMMY + 8) == (BAD_ARG, [SENTINEL])
    assert _color_call(lib, api, f, _tdesc(api, fmt=4)) == (BAD_FORMAT, [SENTINEL])  # the extended call's check comes first
    assert lib.debig_png_decode_batch_tensor_color(None, None, None, None, None, None, None, 0, 0, None, None) == 0
    for desc, fd in ((_tdesc(api), None), (_tdesc(api, flags=1), FD(filter=BILINEAR)), (_tdesc(api, fmt=RGBA | D16, dtype=3), FD(filter=NEAREST)),
                     (_tdesc(api, fmt=RGBA, dtype=1, layout=1), None)):
        assert _color_call(lib, api, f, desc, fd) == (0, [R.E_SIGNATURE])


def test_warp_color_argument_checks_leave_status_unwritten(lib, api):
    f = [b"not a png"]
    bad = [(_tdesc(api), _wdesc(api, filter=BICUBIC)), (_tdesc(api), _wdesc(api, alpha_mode=1)), (_tdesc(api), _wdesc(api, alpha_mode=2)),
           (_tdesc(api), _wdesc(api, border_mode=2)), (_tdesc(api), _wdesc(api, reserved=1)), (_tdesc(api, flags=1), _wdesc(api)),
           (_tdesc(api), _wdesc(api, border=(0, 0, 256, 0))), (_tdesc(api), None), (None, _wdesc(api)),
           (_tdesc(api, fmt=GRAY), _wdesc(api)), (_tdesc(api, fmt=GRAY_ALPHA), _wdesc(api))]
    for desc, wd in bad:
        assert _warp_color_call(lib, api, f, desc, wd) == (BAD_ARG, [SENTINEL]), (desc, wd)
    assert _warp_color_call(lib, api, f, _tdesc(api), _wdesc(api), colors=None) == (BAD_ARG, [SENTINEL])
    assert _warp_color_call(lib, api, f, _tdesc(api), _wdesc(api), warps=None) == (BAD_ARG, [SENTINEL])
    assert _warp_color_call(lib, api, f, _tdesc(api, fmt=4), _wdesc(api)) == (BAD_FORMAT, [SENTINEL])
    assert lib.debig_png_decode_batch_tensor_warp_color(None, None, None, None, None, None, None, None, 0, 0, None, None) == 0
    for desc, wd in ((_tdesc(api), _wdesc(api, filter=NEAREST, border_mode=1)), (_tdesc(api, fmt=RGBA | D16, dtype=2), _wdesc(api, border=(65535,) * 4))):
        assert _warp_color_call(lib, api, f, desc, wd) == (0, [R.E_SIGNATURE])


def test_color_status_is_decided_on_the_host_behind_box_and_warp(lib, api):
    """E_BOX, then E_WARP, then E_COLOR, as soon as IHDR has been read: each outranks what the file holds later (a damaged CRC, a
    missing IDAT); the walk's own statuses before the end of IHDR come first"""
    rng = np.random.default_rng(4)
    rgb = R.encode(R.random_image(rng, 9, 7, 2, 8), 2, 8)
    crc = bytearray(rgb)
    crc[-20] ^= 1
    crc = bytes(crc)
    nanm = list(IDENT)
    nanm[7] = math.nan
    big = list(IDENT)
    big[0] = 16.5
    wnan = (1.0, 0.0, math.nan, 0.0, 1.0, 0.0)
    B, Wp, Cl = Z.E_BOX, WR.E_WARP, CR.E_COLOR
    assert Cl == 17
    files = [rgb, crc, rgb[:40], rgb, rgb[:30], b"\x89PNG", crc]
    boxes = [(0, 0, 10, 1), None, None, None, None, None, (0, 0, 10, 1)]
    colors = [nanm, nanm, big, big, nanm, nanm, IDENT]
    # E_BOX > E_COLOR (0), E_COLOR > a damaged CRC (1), > a missing IDAT (2), a whole file (3); a walk error before the end of IHDR
    # stands (4, 5); E_BOX > a damaged CRC as before (6)
    want = [B, Cl, Cl, Cl, R.E_CHUNK, R.E_SIGNATURE, B]
    assert _color_call(lib, api, files, _tdesc(api), boxes=boxes, colors=colors) == (0, want)
    assert _color_call(lib, api, files, _tdesc(api, fmt=RGBA | D16, flags=1), api.PngFilterDesc(filter=NEAREST), boxes=boxes, colors=colors) == (0, want)
    # with a warp: E_BOX > E_WARP > E_COLOR > later statuses
    warps = [wnan, wnan, WIDENT, wnan, wnan, wnan, WIDENT]
    want = [B, Wp, Cl, Wp, R.E_CHUNK, R.E_SIGNATURE, B]
    assert _warp_color_call(lib, api, files, _tdesc(api), _wdesc(api), boxes=boxes, colors=colors, warps=warps) == (0, want)


# ---- the integer mix against float64 ----------------------------------------------------------------------------------------------

def test_mix_against_float64_on_random_pixels():
    """UINT8, matrices with entries in [-2, 2]: at most one level from round(255 * clip(M x + o, 0, 1)); the bound is derived in
    png_color_ref's docstring from the quantisation steps"""
    rng = np.random.default_rng(23)
    assert CR.float64_bound() == 1
    worst = 0
    for _ in range(60):
        M = rng.uniform(-2, 2, (3, 4))
        px = rng.integers(0, 256, size=(40, 40, 3)).astype(np.uint8)
        got = Z.convert(CR.mix(px.astype(np.int64) << 22, 8, *CR.quantise(M, 8)), 8, "uint").astype(np.int64)
        want = np.floor(255.0 * CR.mix_float64(px / 255.0, M) + 0.5).astype(np.int64)
        worst = max(worst, int(np.abs(got - want).max()))
    print("largest |integer mix - float64| in levels:", worst)
    assert worst <= CR.float64_bound()


def test_mix_consequences_of_the_rule():
    rng = np.random.default_rng(29)
    for P, dt in ((8, np.uint8), (16, np.uint16)):
        px = rng.integers(0, 1 << P, size=(9, 11, 4)).astype(dt)
        px[0, 0] = (1 << P) - 1
        px[0, 1] = 0
        v = px.astype(np.int64) << (30 - P)
        assert np.array_equal(CR.mix(v, P, *CR.quantise(CR.IDENTITY, P)), v)
        perm = [[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]]
        assert np.array_equal(CR.mix(v, P, *CR.quantise(perm, P)), v[:, :, [2, 0, 1, 3]])
        neg = CR.mix(v, P, *CR.quantise(CR.NEGATIVE, P))
        assert np.array_equal(neg[:, :, :3], CR.vmax(P) - v[:, :, :3]) and np.array_equal(neg[:, :, 3], v[:, :, 3])
        assert np.array_equal(Z.convert(neg, P, "uint")[:, :, :3], ((1 << P) - 1) - px[:, :, :3])
        const = CR.mix(v, P, *CR.quantise([[0, 0, 0, 0.25], [0, 0, 0, 2.0], [0, 0, 0, -1.0]], P))
        assert (const[:, :, 0] == CR.quantise([[0, 0, 0, 0.25]] * 3, P)[1][0]).all() and (const[:, :, 1] == CR.vmax(P)).all() and (const[:, :, 2] == 0).all()
        # the extremes of the quantiser stay inside the ranges the header states
        top = CR.mix(v, P, *CR.quantise([[16, 16, 16, 16]] * 3, P))
        assert (top[:, :, :3] <= CR.vmax(P)).all()
