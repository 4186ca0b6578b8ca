"""Output formats of debig_png_decode_batch_fmt (include/decode_png.h) without a GPU: the numpy reference converter of
tests/png_out_format_ref.py on hand-computed pixels, against png_spec_ref.decode (RGBA8) and PIL, and the host-only
debig_png_out_layout against a table."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_out_format_ref as F  # noqa: E402
import png_spec_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------- the converter by hand
def test_gray_weights_and_rounding():
    s = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30], [1, 1, 1]]], np.uint8)
    y = F.convert(s, 2, 8, None, None, F.GRAY)[0, :, 0].tolist()
    # (6968 R + 23434 G + 2366 B + 16384) >> 15
    assert y == [(6968 * 255 + 16384) >> 15, (23434 * 255 + 16384) >> 15, (2366 * 255 + 16384) >> 15,
                 (6968 * 10 + 23434 * 20 + 2366 * 30 + 16384) >> 15, 1]
    assert y == [54, 182, 18, 19, 1]  # 625724 >> 15 = 19


def test_rgb16_to_gray16_and_gray8():
    s = np.array([[[65535, 0, 0], [1000, 40000, 65535], [0x1234, 0x5678, 0x9ABC]]], np.uint16)
    y16 = F.convert(s, 2, 16, None, None, F.GRAY | F.D16)
    assert y16.dtype == np.uint16
    assert y16[0, :, 0].tolist() == [(6968 * 65535 + 16384) >> 15, (6968 * 1000 + 23434 * 40000 + 2366 * 65535 + 16384) >> 15,
                                     (6968 * 0x1234 + 23434 * 0x5678 + 2366 * 0x9ABC + 16384) >> 15]
    # GRAY8 of a 16-bit file: the high bytes first, then the weights
    y8 = F.convert(s, 2, 16, None, None, F.GRAY)
    assert y8.dtype == np.uint8
    assert y8[0, 2, 0] == (6968 * 0x12 + 23434 * 0x56 + 2366 * 0x9A + 16384) >> 15


def test_sub_byte_grey_to_16_bit():
    s1 = np.array([[[1], [0]]], np.uint8)
    assert F.convert(s1, 0, 1, None, None, F.GRAY | F.D16)[0, :, 0].tolist() == [65535, 0]
    s2 = np.array([[[1], [2], [3]]], np.uint8)
    assert F.convert(s2, 0, 2, None, None, F.GRAY | F.D16)[0, :, 0].tolist() == [85 * 257, 170 * 257, 65535]
    assert F.convert(np.array([[[7]]], np.uint8), 0, 4, None, None, F.RGBA | F.D16)[0, 0].tolist() == [7 * 17 * 257] * 3 + [65535]


def test_alpha_rules():
    # colour type 0 with a key: GRAY_ALPHA under NATIVE, alpha 0 on a match, the maximum otherwise
    s = np.array([[[5], [6]]], np.uint16) * 257
    px = F.convert(s, 0, 16, (5 * 257,), None, F.NATIVE | F.D_NATIVE)
    assert px.dtype == np.uint16 and px.tolist() == [[[1285, 0], [1542, 65535]]]
    # an unwanted alpha is dropped, no compositing
    ga = np.array([[[100, 0]]], np.uint8)
    assert F.convert(ga, 4, 8, None, None, F.RGB).tolist() == [[[100, 100, 100]]]
    # a palette: uncovered entries 255; 8 -> 16 is v * 257
    pal = np.array([[10, 20, 30, 7], [40, 50, 60, 255]], np.uint8)
    out = F.convert(np.array([[[0], [1]]], np.uint8), 3, 8, None, pal, F.RGBA | F.D16)
    assert out.tolist() == [[[2570, 5140, 7710, 1799], [10280, 12850, 15420, 65535]]]


def test_resolve_table():
    assert F.resolve(0, 1, 0, F.NATIVE | F.D_NATIVE) == (F.GRAY, 8)
    assert F.resolve(0, 16, 1, F.NATIVE | F.D_NATIVE) == (F.GRAY_ALPHA, 16)
    assert F.resolve(4, 8, 0, F.NATIVE) == (F.GRAY_ALPHA, 8)
    assert F.resolve(2, 16, 0, F.NATIVE | F.D_NATIVE) == (F.RGB, 16)
    assert F.resolve(3, 4, 1, F.NATIVE | F.D_NATIVE) == (F.RGBA, 8)
    assert F.resolve(3, 8, 0, F.NATIVE | F.D16) == (F.RGB, 16)
    assert F.resolve(6, 16, 0, F.GRAY) == (F.GRAY, 8)


# ------------------------------------------------------------------------------------------- against png_spec_ref
def _cases():
    rng = np.random.default_rng(31)
    for ct, depths in R.DEPTHS.items():
        for depth in depths:
            for il in (0, 1):
                for trns in ((0, 1) if ct in (0, 2, 3) else (0,)):
                    w, h = 11 + il * 6, 9
                    pal = t = None
                    if ct == 3:
                        n_pal = max(2, (1 << depth) - 1)
                        pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n_pal)]
                        s = R.random_image(rng, w, h, ct, depth, n_pal)
                        if trns:
                            t = bytes(rng.integers(0, 256, size=n_pal - 1, dtype=np.uint8))
                    else:
                        s = R.random_image(rng, w, h, ct, depth)
                        if trns:
                            s = s % 3 if depth != 16 else (s % 3) * 257
                            t = np.asarray(s[0, 0][: 3 if ct == 2 else 1], dtype=">u2").tobytes()
                    yield (ct, depth, il, trns), R.encode(s, ct, depth, il, trns=t, palette=pal)


CASES = list(_cases())


@pytest.mark.parametrize("key,data", CASES, ids=[str(k) for k, _ in CASES])
def test_format_zero_is_the_rgba8_reference(key, data):
    st, px, _ = F.decode(data, 0)
    est, epx, _ = R.decode(data)
    assert st == est == R.OK
    assert px.dtype == np.uint8 and np.array_equal(px, epx)


@pytest.mark.parametrize("key,data", CASES, ids=[str(k) for k, _ in CASES])
def test_every_format_is_consistent(key, data):
    """16-bit output reduced to its high byte is the 8-bit output; RGBA8 carries the RGB8 channels; NATIVE is one of
    the concrete layouts"""
    ct, depth, il, trns = key
    rgba8 = F.decode(data, F.RGBA)[1]
    assert np.array_equal(F.decode(data, F.RGB)[1], rgba8[:, :, :3])
    for lay in (F.RGBA, F.RGB, F.GRAY, F.GRAY_ALPHA, F.NATIVE):
        p8 = F.decode(data, lay)[1]
        p16 = F.decode(data, lay | F.D16)[1]
        assert p16.dtype == np.uint16 and p8.dtype == np.uint8
        if lay in (F.RGBA, F.RGB, F.NATIVE):  # no weights: reduction and the layout commute
            assert np.array_equal((p16 >> 8).astype(np.uint8), p8)
        if depth != 16:  # an 8-bit source: 16-bit output is v * 257 for copied samples
            if lay in (F.RGBA, F.RGB, F.NATIVE):
                assert np.array_equal(p16, p8.astype(np.uint16) * 257)
    nat = F.decode(data, F.NATIVE | F.D_NATIVE)[1]
    assert nat.dtype == (np.uint16 if depth == 16 else np.uint8)
    assert nat.shape[2] == {0: 2 if trns else 1, 4: 2, 2: 4 if trns else 3, 3: 4 if trns else 3, 6: 4}[ct]


# ------------------------------------------------------------------------------------------- against PIL
def _pil():
    return pytest.importorskip("PIL.Image")


def _pil_png(img, **kw):
    b = io.BytesIO()
    img.save(b, format="PNG", **kw)
    return b.getvalue()


@pytest.mark.parametrize("mode", ["L", "LA", "RGB", "RGBA", "P", "P+tRNS"])
def test_native_8bit_matches_pil(mode):
    Image = _pil()
    rng = np.random.default_rng(3)
    if mode.startswith("P"):
        img = Image.fromarray(rng.integers(0, 40, size=(13, 17), dtype=np.uint8), "L").convert("P")
        img.putpalette(list(rng.integers(0, 256, size=3 * 40).astype(int)))
        kw = {"transparency": bytes(rng.integers(0, 256, size=20, dtype=np.uint8))} if mode == "P+tRNS" else {}
        data = _pil_png(img, **kw)
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA" if kw else "RGB"))
    else:
        ch = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
        arr = rng.integers(0, 256, size=(13, 17, ch), dtype=np.uint8)
        data = _pil_png(Image.fromarray(arr[:, :, 0] if ch == 1 else arr, mode))
        want = np.asarray(Image.open(io.BytesIO(data)))
        if want.ndim == 2:
            want = want[:, :, None]
    st, px, _ = F.decode(data, F.NATIVE)
    assert st == R.OK
    assert px.shape == want.shape and np.array_equal(px, want)


def test_gray16_matches_pil_i16():
    Image = _pil()
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 65536, size=(9, 14), dtype=np.uint16)
    data = R.encode(arr[:, :, None], 0, 16)
    want = np.asarray(Image.open(io.BytesIO(data)))
    assert Image.open(io.BytesIO(data)).mode == "I;16"
    for fmt in (F.NATIVE | F.D_NATIVE, F.GRAY | F.D16):
        st, px, _ = F.decode(data, fmt)
        assert st == R.OK and px.dtype == np.uint16
        assert np.array_equal(px[:, :, 0], want.astype(np.uint16))
        assert px.tobytes() == arr.astype("<u2").tobytes()  # little-endian in memory


# ------------------------------------------------------------------------------------------- debig_png_out_layout
class PngInfo(C.Structure):  # include/decode_png.h: debig_png_info
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8), ("color_type", C.c_uint8),
                ("interlace", C.c_uint8), ("has_trns", C.c_uint8), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_out_layout.restype = C.c_uint64
    L.debig_png_out_layout.argtypes = [C.POINTER(PngInfo), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.debig_png_decode_batch_fmt.restype = C.c_int
    L.debig_png_decode_batch_fmt.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32]
    return L


def test_out_layout_table(lib):
    for ct, depths in R.DEPTHS.items():
        for depth in depths:
            for trns in (0, 1):
                for il in (0, 1):
                    inf = PngInfo(width=0x7FFFFFFF if depth == 16 else 3, height=0x7FFFFFFF if depth == 16 else 5,
                                  bit_depth=depth, color_type=ct, interlace=il, has_trns=trns)
                    for fmt in F.FORMATS:
                        ch, bs = C.c_uint32(99), C.c_uint32(99)
                        n = lib.debig_png_out_layout(C.byref(inf), fmt, C.byref(ch), C.byref(bs))
                        wch, wbs, wn = F.layout(inf.width, inf.height, ct, depth, trns, fmt)
                        assert (ch.value, bs.value, n) == (wch, wbs, min(wn, 2 ** 64 - 1)), (ct, depth, trns, fmt)
    # 64-bit sizes: 4 * (2^31 - 1)^2 fits, 8 * (2^31 - 1)^2 saturates
    inf = PngInfo(width=0x7FFFFFFF, height=0x7FFFFFFF, bit_depth=16, color_type=6)
    assert lib.debig_png_out_layout(C.byref(inf), F.RGBA, None, None) == 4 * 0x7FFFFFFF ** 2
    assert lib.debig_png_out_layout(C.byref(inf), F.RGBA | F.D16, None, None) == 2 ** 64 - 1


@pytest.mark.parametrize("fmt", [5, 6, 15, 0x30, 0x34, 0x40, 0x100, 0x80000000, 0xFFFFFFFF, 0x15])
def test_out_layout_and_decode_reject_bad_formats(lib, fmt):
    inf = PngInfo(width=4, height=4, bit_depth=8, color_type=6)
    ch, bs = C.c_uint32(99), C.c_uint32(99)
    assert lib.debig_png_out_layout(C.byref(inf), fmt, C.byref(ch), C.byref(bs)) == 0
    assert (ch.value, bs.value) == (99, 99)
    # DEBIG_PNG_BAD_FORMAT, and nothing written (the file would fail on the host anyway: no device work here)
    st = (C.c_uint32 * 1)(0xABCD)
    buf = C.create_string_buffer(b"not a png", 9)
    out = C.create_string_buffer(64)
    rc = lib.debig_png_decode_batch_fmt((C.c_void_p * 1)(C.addressof(buf)), (C.c_uint64 * 1)(9),
                                        (C.c_void_p * 1)(C.addressof(out)), (C.c_uint64 * 1)(64), st, None, 1, 0, fmt)
    assert rc == -1
    assert st[0] == 0xABCD


def test_out_layout_invalid_info(lib):
    inf = PngInfo(width=4, height=4, bit_depth=3, color_type=6)
    assert lib.debig_png_out_layout(C.byref(inf), 0, None, None) == 0
    assert lib.debig_png_out_layout(None, 0, None, None) == 0


def test_host_statuses_under_every_format(lib):
    """files that fail on the host report the same status under every format; E_OUTPUT follows the format's size"""
    good = R.encode(np.zeros((5, 7, 1), np.uint8), 0, 8)
    bad_sig = b"\x00" + good[1:]
    for fmt in F.FORMATS:
        datas = [bad_sig, good]
        bufs = [C.create_string_buffer(d, len(d)) for d in datas]
        outs = [C.create_string_buffer(512) for _ in datas]
        st = (C.c_uint32 * 2)()
        need = F.layout(7, 5, 0, 8, 0, fmt)[2]
        rc = lib.debig_png_decode_batch_fmt((C.c_void_p * 2)(*[C.addressof(b) for b in bufs]),
                                            (C.c_uint64 * 2)(*[len(d) for d in datas]),
                                            (C.c_void_p * 2)(*[C.addressof(o) for o in outs]),
                                            (C.c_uint64 * 2)(512, need - 1), st, None, 2, 0, fmt)
        assert rc == 0
        assert list(st) == [R.E_SIGNATURE, R.E_OUTPUT], fmt
