"""The alpha arithmetic of debig_png_decode_batch_tensor_alpha (include/decode_png.h) without a GPU: the numpy restatement
(tests/png_alpha_ref.py) against a float64 model on the same Q14 weights, the opaque and transparent identities, and the
argument checks of the C call and of the Python call (they are decided before any file is looked at and before any device
work)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_alpha_ref as A  # noqa: E402
import png_resize_ref as Z  # noqa: E402
import png_spec_ref as R  # noqa: E402

BAD_FORMAT, BAD_ARG = -1, -2
DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
RGBA, RGB, GRAY, GRAY_ALPHA = 0, 1, 2, 3


class Desc(C.Structure):  # include/decode_png.h: debig_png_tensor_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("out_format", C.c_uint32), ("out_layout", C.c_uint32),
                ("dtype", C.c_uint32), ("resize_flags", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class AlphaDesc(C.Structure):  # include/decode_png.h: debig_png_alpha_desc
    _fields_ = [("mode", C.c_uint32), ("background", C.c_uint16 * 4), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_decode_batch_tensor_alpha.restype = C.c_int
    L.debig_png_decode_batch_tensor_alpha.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


# ---- the restatement against real arithmetic ------------------------------------------------------------------------------

def _exact(px, size, aa, box, mode, bg):
    """premultiply, filter and composite in float64 on the SAME Q14 weights (as exact fractions w / 16384) -> the output
    samples on the 0 .. M scale, unrounded"""
    P = 8 * px.dtype.itemsize
    M = float((1 << P) - 1)
    if box is not None:
        x, y, w, h = box
        px = px[y:y + h, x:x + w]
    h, w, Cn = px.shape
    H, W = size
    s = px.astype(np.float64)
    p = s.copy()
    p[:, :, :-1] = s[:, :, :-1] * s[:, :, -1:] / M
    hq = np.empty((h, W, Cn))
    for X, (f, wt) in enumerate(Z.axis(w, W, aa)):
        hq[:, X, :] = np.tensordot(p[:, f:f + len(wt), :], np.array(wt, np.float64) / Z.ONE, axes=([1], [0]))
    v = np.empty((H, W, Cn))
    for Y, (f, wt) in enumerate(Z.axis(h, H, aa)):
        v[Y] = np.tensordot(np.array(wt, np.float64) / Z.ONE, hq[f:f + len(wt)], axes=([0], [0]))
    if mode == A.PREMULTIPLIED:
        return v
    return v[:, :, :-1] + np.asarray(bg[:Cn - 1], np.float64) * (M - v[:, :, -1:]) / M


CASES = [  # (h, w), (H, W), box
    ((3, 5), (7, 9), None), ((64, 48), (17, 23), None), ((100, 37), (37, 100), None), ((90, 120), (224, 224), None),
    ((300, 400), (64, 64), (10, 20, 333, 250)), ((1, 9), (4, 3), None), ((50, 60), (1, 1), None), ((41, 67), (41, 67), None),
    ((512, 512), (112, 112), None), ((77, 130), (200, 30), (3, 4, 120, 70)),
]


@pytest.mark.parametrize("mode", [A.OVER, A.PREMULTIPLIED])
@pytest.mark.parametrize("Cn", [4, 2])
@pytest.mark.parametrize("P", [8, 16])
@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("src,size,box", CASES)
def test_restatement_against_a_float64_model_on_the_same_weights(src, size, box, aa, P, Cn, mode):
    """The bound is derived from the rounding steps, in units of one output sample (full scale M = 2^P - 1); the weights of
    an axis are >= 0 and sum to exactly 1, so an error of at most e on every input of a pass is at most e on its output.
      - premultiply: p_c is the exact s_c * alpha / M rounded to an integer: <= 0.5 on colour, none on alpha;
      - Hq keeps 16 bits of a sample times 2^14, i.e. the sample times 2^(16 - P), rounded to nearest: <= 0.5 / 2^(16 - P)
        = 2^-9 (P = 8) or 0.5 (P = 16), once on colour and once on alpha;
      - the vertical pass is exact in 30 bits; so is t = Vmax - v_alpha;
      - the composite adds b_c * t / M rounded in the 30-bit domain: <= 0.5 / 2^(30 - P) (< 2^-15), and carries alpha's
        error times b_c / M <= 1;
      - the final conversion rounds to an integer: <= 0.5.
    OVER:  P = 8: 0.5 + 2^-9 + 2^-9 + 2^-23 + 0.5 < 1.01;   P = 16: 0.5 + 0.5 + 0.5 + 2^-15 + 0.5 < 2.01.
    PREMULTIPLIED has the colour terms only and stays under the same bounds.  Observed on the cases below: 0.97 (P = 8) and 1.74 (P = 16) in OVER
    mode, 0.97 and 1.41 in PREMULTIPLIED mode."""
    rng = np.random.default_rng(src[0] * 7 + src[1] + size[0] + P + Cn)
    M = (1 << P) - 1
    px = rng.integers(0, M + 1, size=(src[0], src[1], Cn), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    px[: src[0] // 2, : src[1] // 3, :-1] = M
    px[src[0] // 3:, src[1] // 2:, -1] = rng.choice([0, 1, M - 1, M], size=px[src[0] // 3:, src[1] // 2:, -1].shape)
    bg = [M, M // 3, 0]
    got = A.resize_alpha(px, size, mode, "uint", aa, box, background=bg).astype(np.float64)
    err = float(np.abs(got - _exact(px, size, aa, box, mode, bg)).max())
    bound = 1.01 if P == 8 else 2.01
    print(f"P {P} mode {mode}: max |uint output - exact| {err:.4f}, bound {bound}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("Cn", [4, 2])
@pytest.mark.parametrize("P", [8, 16])
def test_opaque_and_transparent_identities(P, Cn):
    rng = np.random.default_rng(P + Cn)
    M = (1 << P) - 1
    px = rng.integers(0, M + 1, size=(61, 83, Cn), dtype=np.uint16).astype(np.uint8 if P == 8 else np.uint16)
    opaque, clear = px.copy(), px.copy()
    opaque[:, :, -1] = M
    clear[:, :, -1] = 0
    for aa in (True, False):
        for size, box in (((17, 23), None), ((61, 83), None), ((90, 40), (5, 6, 50, 31))):
            for bg in ([0] * 3, [M] * 3, [1, M // 2, M - 1]):
                v, _ = A.resize_alpha_int(opaque, size, A.OVER, aa, box, bg)
                assert np.array_equal(v, Z.resize_int(opaque[:, :, :-1], size, aa, box)[0])  # today's mode="rgb" / "gray"
                v, _ = A.resize_alpha_int(clear, size, A.OVER, aa, box, bg)
                assert (v == (np.array(bg[:Cn - 1], np.int64) << (30 - P))).all()  # b_c << S exactly
            v, _ = A.resize_alpha_int(opaque, size, A.PREMULTIPLIED, aa, box)
            assert np.array_equal(v, Z.resize_int(opaque, size, aa, box)[0])  # today's mode="rgba" / "gray_alpha"
            v, _ = A.resize_alpha_int(px, size, A.PREMULTIPLIED, aa, box)
            assert (v[:, :, :-1] <= v[:, :, -1:]).all() and v.max() <= M << (30 - P)


def test_premultiply_rule():
    px = np.array([[[255, 128, 1, 255], [255, 128, 1, 0], [255, 128, 1, 1], [200, 100, 3, 128]]], np.uint8)
    assert A.premultiply(px).tolist() == [[[255, 128, 1, 255], [0, 0, 0, 0], [1, 1, 0, 1], [100, 50, 2, 128]]]
    px16 = np.array([[[65535, 65535], [40000, 32768], [3, 1]]], np.uint16)
    assert A.premultiply(px16).tolist() == [[[65535, 65535], [(40000 * 32768 + 32767) // 65535, 32768], [0, 1]]]
    # the kernel's 32-bit form of the composite's division: t = q M + r
    rng = np.random.default_rng(1)
    for P in (8, 16):
        M = (1 << P) - 1
        t = rng.integers(0, (M << (30 - P)) + 1, size=100000)
        b = rng.integers(0, M + 1, size=100000)
        q, r = t // M, t % M
        assert (b * r + (M >> 1)).max() < 1 << 32
        assert np.array_equal((b * t + (M >> 1)) // M, b * q + (b * r + (M >> 1)) // M)


# ---- the C call's checks (no GPU: everything below returns before any device work) ---------------------------------------

def _desc(**kw):
    d = Desc(out_w=8, out_h=8, out_format=RGB, out_layout=1, dtype=1, resize_flags=1)
    for k in range(4):
        d.scale[k], d.bias[k] = 1.0, 0.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _alpha(mode, background=(0, 0, 0, 0), reserved=0):
    return AlphaDesc(mode=mode, background=(C.c_uint16 * 4)(*background), reserved=reserved)


def _call(lib, files, desc, alpha, out=DUMMY):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[0xABCD] * n)
    rc = lib.debig_png_decode_batch_tensor_alpha(ins, sizes, out, None, st, None, n, 0, C.byref(desc) if desc is not None else None,
                                                 C.byref(alpha) if alpha is not None else None)
    return rc, list(st)


REFUSED = [
    # a mode / layout pairing other than OVER + RGB / GRAY and PREMULTIPLIED + RGBA / GRAY_ALPHA
    (dict(out_format=RGBA), _alpha(A.OVER)), (dict(out_format=GRAY_ALPHA), _alpha(A.OVER)),
    (dict(out_format=RGBA | 0x10), _alpha(A.OVER)), (dict(out_format=RGB), _alpha(A.PREMULTIPLIED)),
    (dict(out_format=GRAY), _alpha(A.PREMULTIPLIED)), (dict(out_format=GRAY | 0x10), _alpha(A.PREMULTIPLIED)),
    # an unknown mode, reserved != 0 (whatever the mode)
    (dict(), _alpha(3)), (dict(), _alpha(0xFFFFFFFF)), (dict(out_format=RGBA), _alpha(7)),
    (dict(), _alpha(A.OVER, reserved=1)), (dict(out_format=RGBA), _alpha(A.PREMULTIPLIED, reserved=0x80000000)),
    (dict(), _alpha(A.STRAIGHT, reserved=2)),
    # OVER: a used background sample above 2^P - 1
    (dict(out_format=RGB), _alpha(A.OVER, (256, 0, 0, 0))), (dict(out_format=RGB), _alpha(A.OVER, (0, 0, 65535, 0))),
    (dict(out_format=GRAY), _alpha(A.OVER, (300, 0, 0, 0))),
]


@pytest.mark.parametrize("kw,alpha", REFUSED)
def test_bad_alpha_descriptors_are_refused_before_any_file(lib, kw, alpha):
    rc, st = _call(lib, [b"not a png"] * 2, _desc(**kw), alpha)
    assert rc == BAD_ARG and st == [0xABCD] * 2


def test_the_existing_checks_come_first_and_unchanged(lib):
    for kw, want in ((dict(out_format=4), BAD_FORMAT), (dict(out_format=0x20), BAD_FORMAT), (dict(out_layout=2), BAD_FORMAT),
                     (dict(dtype=4), BAD_ARG), (dict(resize_flags=2), BAD_ARG), (dict(out_w=0), BAD_ARG), (dict(out_h=16385), BAD_ARG)):
        for alpha in (None, _alpha(A.OVER), _alpha(3), _alpha(A.PREMULTIPLIED)):
            assert _call(lib, [b"not a png"], _desc(**kw), alpha) == (want, [0xABCD]), (kw, alpha)
    assert _call(lib, [b"not a png"], None, _alpha(A.OVER)) == (BAD_ARG, [0xABCD])
    assert _call(lib, [b"not a png"], _desc(), _alpha(A.OVER), out=None) == (BAD_ARG, [0xABCD])
    assert _call(lib, [b"not a png"], _desc(), _alpha(A.OVER), out=DUMMY + 8) == (BAD_ARG, [0xABCD])
    d = _desc()
    d.scale[1] = float("inf")
    assert _call(lib, [b"not a png"], d, _alpha(A.OVER)) == (BAD_ARG, [0xABCD])
    assert lib.debig_png_decode_batch_tensor_alpha(None, None, None, None, None, None, 0, 0, None, None) == 0  # n == 0


def test_accepted_descriptors_reach_the_files(lib):
    """alpha == NULL, STRAIGHT with any layout, and every valid pairing pass the checks: the files are looked at (both are
    broken before IHDR ends, so no device work follows)"""
    rng = np.random.default_rng(1)
    png = R.encode(R.random_image(rng, 40, 30, 6, 8), 6, 8)
    files = [b"not a png", png[:30]]
    want = (0, [R.E_SIGNATURE, R.E_CHUNK])
    for fmt in (RGBA, RGB, GRAY, GRAY_ALPHA, RGB | 0x10):
        assert _call(lib, files, _desc(out_format=fmt), None) == want
        assert _call(lib, files, _desc(out_format=fmt), _alpha(A.STRAIGHT, (999, 999, 999, 999))) == want
    for fmt in (RGB, GRAY):
        assert _call(lib, files, _desc(out_format=fmt), _alpha(A.OVER, (255, 255, 255, 0) if fmt == RGB else (255, 0, 0, 0))) == want
        assert _call(lib, files, _desc(out_format=fmt | 0x10), _alpha(A.OVER, (65535, 256, 65535, 65535))) == want
    assert _call(lib, files, _desc(out_format=RGB), _alpha(A.OVER, (0, 255, 1, 999))) == want   # background[3] is not used
    assert _call(lib, files, _desc(out_format=GRAY), _alpha(A.OVER, (255, 999, 999, 999))) == want
    for fmt in (RGBA, GRAY_ALPHA, RGBA | 0x10, GRAY_ALPHA | 0x10):
        assert _call(lib, files, _desc(out_format=fmt), _alpha(A.PREMULTIPLIED, (999, 999, 999, 999))) == want  # unused


def test_box_rule_is_the_tensor_calls(lib):
    rng = np.random.default_rng(2)
    png = R.encode(R.random_image(rng, 40, 30, 6, 8), 6, 8)
    n = 3
    bufs = [C.create_string_buffer(f, len(f)) for f in (png, png[:60], b"not a png")]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(len(png), 60, 9)
    st = (C.c_uint32 * n)(*[0xABCD] * n)
    boxes = (C.c_uint32 * 12)(36, 0, 5, 5, 0, 0, 41, 1, 0, 0, 5, 0)
    d, a = _desc(), _alpha(A.OVER, (255, 255, 255, 0))
    rc = lib.debig_png_decode_batch_tensor_alpha(ins, sizes, DUMMY, boxes, st, None, n, 0, C.byref(d), C.byref(a))
    assert rc == 0 and list(st) == [Z.E_BOX, Z.E_BOX, R.E_SIGNATURE]


def test_python_arguments():
    from debigulator_amd import api

    assert api.png_alpha_desc() is None and api.png_alpha_desc("straight", mode="rgba") is None
    d = api.png_alpha_desc("over")
    assert (d.mode, list(d.background), d.reserved) == (2, [255, 255, 255, 0], 0)  # white
    d = api.png_alpha_desc("over", [0.0, 0.5, 1.0], mode="rgb", depth=16)
    assert list(d.background) == [0, round(0.5 * 65535), 65535, 0]
    d = api.png_alpha_desc("over", 0.25, mode="gray")
    assert (d.mode, list(d.background)) == (2, [64, 0, 0, 0])
    assert list(api.png_alpha_desc("over", (0.2, 0.4, 0.6)).background) == A.background_samples((0.2, 0.4, 0.6), 3, 8) + [0]
    d = api.png_alpha_desc("premultiplied", mode="gray_alpha", depth=16)
    assert (d.mode, list(d.background), d.reserved) == (1, [0, 0, 0, 0], 0)
    assert C.sizeof(api.PngAlphaDesc) == C.sizeof(AlphaDesc) == 16
    for kw in (dict(alpha="under"), dict(alpha="over", mode="rgba"), dict(alpha="over", mode="gray_alpha"),
               dict(alpha="premultiplied", mode="rgb"), dict(alpha="premultiplied", mode="gray"),
               dict(alpha="over", background=[1.0, 1.0]), dict(alpha="over", background=[0.0, 1.5, 0.0]),
               dict(alpha="over", background=-0.01), dict(alpha="over", background=float("nan")),
               dict(alpha="over", background=[0.5], mode="rgb"), dict(alpha="premultiplied", mode="rgba", background=1.0),
               dict(alpha="straight", background=1.0), dict(alpha="over", depth="native"), dict(alpha="over", mode="native")):
        with pytest.raises(ValueError):
            api.png_alpha_desc(**kw)
    for kw in (dict(mode="rgba", alpha="over"), dict(mode="rgb", alpha="premultiplied"), dict(alpha="over", background=2.0),
               dict(alpha="sideways")):
        with pytest.raises(ValueError):  # (raised before the library or a device is touched)
            api.png_decode_batch_tensor([b"not a png"], (8, 8), **kw)
    import inspect

    sig = inspect.signature(api.png_decode_batch_tensor).parameters
    assert sig["alpha"].default == "straight" and sig["background"].default is None


def test_symbols_are_exported(lib):
    from debigulator_amd import _native as N

    out = os.popen(f"nm -D --defined-only {N.LIB_PATH}").read()
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"debig_png_decode_batch_tensor_alpha", "debig_hip_png_resize_alpha_batch", "debig_png_decode_batch_tensor"} <= syms
