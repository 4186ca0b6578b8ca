"""debig_png_decode_batch_fmt on the MI355X (include/decode_png.h): every (colour type, depth, interlace, tRNS) to every
output format against the numpy converter of tests/png_out_format_ref.py, format 0 against debig_png_decode_batch,
the resource PNGs in NATIVE against PIL, E_OUTPUT at the exact size, every error status under other formats, size
extremes, and the Python dtypes and shapes."""
import ctypes as C
import glob
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_out_format_ref as F  # noqa: E402
import png_spec_ref as R  # noqa: E402
import test_gpu_png_spec as G  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "resources", "*.png")))
MODE_DEPTHS = [(F.MODES[f & 15], F.DEPTHS[f & 0x30]) for f in F.FORMATS]


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A

    return A


@pytest.fixture(scope="module")
def files():
    fs = G._all_formats()
    return fs, [F.decode(d, 0)[2] for _, d in fs]


def _check(out, datas, fmt):
    for data, (st, px, inf) in zip(datas, out):
        est, epx, einf = F.decode(data, fmt)
        assert est == R.OK
        assert st == 0, (einf, hex(fmt), st)
        assert inf == einf
        assert px.dtype == epx.dtype and px.shape == epx.shape, (einf, hex(fmt))
        assert np.array_equal(px, epx), (einf, hex(fmt), np.argwhere(px != epx)[:4])


@pytest.mark.parametrize("mode,depth", MODE_DEPTHS)
def test_every_format_in_one_mixed_batch(api, files, mode, depth):
    fs, _ = files
    datas = [d for _, d in fs]
    _check(api.png_decode_batch(datas, mode=mode, depth=depth), datas, api.png_out_format(mode, depth))


@pytest.mark.parametrize("mode,depth", [("gray", 16), ("rgb", 8), ("native", "native"), ("gray_alpha", 8)])
def test_every_format_one_file_at_a_time(api, files, mode, depth):
    fs, _ = files
    fmt = api.png_out_format(mode, depth)
    for _, d in fs:
        _check(api.png_decode_batch([d], mode=mode, depth=depth), [d], fmt)
        _check(api.png_decode_batch([d], mode=mode, depth=depth, force_general=True), [d], fmt)


def _raw_fmt(api, datas, fmt, flags=0, caps=None, old=False):
    """debig_png_decode_batch(_fmt) with caps of the exact size -> (statuses, [bytes])"""
    from debigulator_amd import _native as N

    L = api._png_spec_lib()
    n = len(datas)
    ins = [np.frombuffer(d, np.uint8) for d in datas]
    if caps is None:
        caps = [api.png_out_layout(api.png_info(d)[1], F.MODES[fmt & 15], F.DEPTHS[fmt & 0x30])[2] for d in datas]
    outs = [np.full(c + 64, 0xA5, np.uint8) for c in caps]
    st = (C.c_uint32 * n)()
    args = [(C.c_void_p * n)(*[a.ctypes.data for a in ins]), (C.c_uint64 * n)(*[len(d) for d in datas]),
            (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_uint64 * n)(*caps), st, None, n, flags]
    rc = L.debig_png_decode_batch(*args) if old else L.debig_png_decode_batch_fmt(*args, fmt)
    N.check(rc, "debig_png_decode_batch_fmt")
    for o, c in zip(outs, caps):
        assert (o[c:] == 0xA5).all(), "written past the capacity"
    return list(st), [o[:c].tobytes() for o, c in zip(outs, caps)]


def test_format_zero_is_debig_png_decode_batch(api, files):
    fs, _ = files
    datas = [d for _, d in fs]
    rng = np.random.default_rng(3)
    datas += [R.encode(R.random_image(rng, w, 37, ct, 8), ct, 8) for ct in (2, 6) for w in (1, 64, 333)]  # tuned routing
    for flags in (0, api.PNG_FORCE_GENERAL):
        sa, a = _raw_fmt(api, datas, 0, flags, old=True)
        sb, b = _raw_fmt(api, datas, 0, flags)
        assert sa == sb == [0] * len(datas)
        assert a == b


def test_native_rgba8_of_tuned_files_is_the_tuned_output(api):
    """NATIVE of an 8-bit RGBA file resolves to RGBA8, so it takes the tuned routing: the same bytes"""
    rng = np.random.default_rng(4)
    datas = [R.encode(R.random_image(rng, 200, 70, 6, 8), 6, 8), R.encode(R.random_image(rng, 31, 9, 2, 8), 2, 8)]
    a = api.png_decode_batch(datas)
    b = api.png_decode_batch(datas, mode="native", depth="native")
    assert np.array_equal(a[0][1], b[0][1])
    assert np.array_equal(a[1][1][:, :, :3], b[1][1])


def test_resource_files_native_match_pil(api):
    Image = pytest.importorskip("PIL.Image")
    datas = [open(p, "rb").read() for p in RESOURCES]
    assert len(datas) == 15
    out = api.png_decode_batch(datas, mode="native", depth="native")
    for p, data, (st, px, inf) in zip(RESOURCES, datas, out):
        assert st == 0, p
        im = Image.open(io.BytesIO(data))
        if inf["color_type"] == 3:
            want = np.asarray(im.convert("RGBA" if inf["has_trns"] else "RGB"))
        elif inf["bit_depth"] == 16 or inf["color_type"] in (0, 2) and inf["has_trns"]:
            want = F.decode(data, F.NATIVE | F.D_NATIVE)[1]  # PIL has no mode for these
        else:
            want = np.asarray(im)
        if want.ndim == 2:
            want = want[:, :, None]
        assert px.shape == want.shape and np.array_equal(px, want), p
        assert np.array_equal(px, F.decode(data, F.NATIVE | F.D_NATIVE)[1]), p


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_output_capacity_exact_and_one_less(api, fmt):
    rng = np.random.default_rng(8)
    datas = [R.encode(R.random_image(rng, 13, 9, 2, 16), 2, 16), R.encode(R.random_image(rng, 13, 9, 0, 4), 0, 4, 1)]
    exact = [api.png_out_layout(api.png_info(d)[1], F.MODES[fmt & 15], F.DEPTHS[fmt & 0x30])[2] for d in datas]
    st, outs = _raw_fmt(api, datas, fmt, caps=exact)
    assert st == [0, 0]
    for d, o in zip(datas, outs):
        assert o == F.decode(d, fmt)[1].tobytes()
    st, _ = _raw_fmt(api, datas, fmt, caps=[exact[0] - 1, exact[1]])
    assert st == [R.E_OUTPUT, 0]
    st, _ = _raw_fmt(api, datas, fmt, caps=[exact[0], exact[1] - 1])
    assert st == [0, R.E_OUTPUT]


@pytest.mark.parametrize("mode,depth", [("gray", 16), ("rgb", 8), ("native", "native")])
def test_error_statuses_under_other_formats(api, mode, depth):
    cases = G._error_files()
    fs = G._all_formats()[::3]
    batch, expect = [], []
    for k, (name, data, st) in enumerate(cases):
        batch += [data, fs[k % len(fs)][1]]
        expect += [(name, st), ("good", 0)]
    out = api.png_decode_batch(batch, mode=mode, depth=depth)
    fmt = api.png_out_format(mode, depth)
    for data, (name, st), (got, px, _) in zip(batch, expect, out):
        assert got == st, (name, got)
        if st == 0:
            assert np.array_equal(px, F.decode(data, fmt)[1])
    for name, data, st in cases:
        assert api.png_decode_batch([data], mode=mode, depth=depth)[0][0] == st, name


def test_size_extremes(api):
    rng = np.random.default_rng(9)
    one = R.encode(np.array([[[7, 8, 9, 10]]], np.uint8), 6, 8)
    one_il = R.encode(np.array([[[40000]]], np.uint16), 0, 16, 1, trns=b"\x9c\x40")
    wide = R.encode(R.random_image(rng, 16384, 3, 0, 1), 0, 1, filters=lambda p, y: (1, 4, 3)[y])
    datas = [one, one_il, wide]
    for mode, depth in MODE_DEPTHS:
        out = api.png_decode_batch(datas, mode=mode, depth=depth)
        _check(out, datas, api.png_out_format(mode, depth))
    assert api.png_decode_batch([one_il], mode="native", depth="native")[0][1].tolist() == [[[40000, 0]]]
    # 4096 x 4096 16-bit RGBA, every row filter type 0 (scanlines made here, so the expected pixels are the samples)
    import zlib

    s = rng.integers(0, 65536, size=(4096, 4096, 4), dtype=np.uint16)
    rows = np.zeros((4096, 1 + 4096 * 8), np.uint8)
    rows[:, 1:] = s.astype(">u2").reshape(4096, -1).view(np.uint8)
    big = R.encode(s[:1, :1], 6, 16, zdata=zlib.compress(rows.tobytes(), 1),
                   ihdr=np.array([4096, 4096], ">u4").tobytes() + bytes([16, 6, 0, 0, 0]))
    del rows
    st, px, _ = api.png_decode_batch([big], mode="rgba", depth=16)[0]
    assert st == 0 and px.dtype == np.uint16 and np.array_equal(px, s)
    st, px, _ = api.png_decode_batch([big], mode="rgb", depth=8)[0]
    assert st == 0 and np.array_equal(px, (s[:, :, :3] >> 8).astype(np.uint8))
    st, px, _ = api.png_decode_batch([big], mode="gray", depth=16)[0]
    y = (6968 * s[:, :, 0].astype(np.uint32) + 23434 * s[:, :, 1].astype(np.uint32) + 2366 * s[:, :, 2].astype(np.uint32)
         + 16384) >> 15
    assert st == 0 and np.array_equal(px[:, :, 0], y.astype(np.uint16))


def test_python_dtype_and_shape(api):
    rng = np.random.default_rng(10)
    d16 = R.encode(R.random_image(rng, 5, 3, 4, 16), 4, 16)
    d8 = R.encode(R.random_image(rng, 5, 3, 0, 8), 0, 8)
    want = {("rgba", 8): (4, np.uint8), ("rgb", 8): (3, np.uint8), ("gray", 8): (1, np.uint8),
            ("gray_alpha", 16): (2, np.uint16), ("rgba", 16): (4, np.uint16)}
    for (mode, depth), (ch, dt) in want.items():
        for d in (d16, d8):
            st, px, _ = api.png_decode_batch([d], mode=mode, depth=depth)[0]
            assert st == 0 and px.shape == (3, 5, ch) and px.dtype == dt
    assert api.png_decode_batch([d16], mode="native", depth="native")[0][1].dtype == np.uint16
    assert api.png_decode_batch([d8], mode="native", depth="native")[0][1].shape == (3, 5, 1)
    assert api.png_decode_batch([d16])[0][1].shape == (3, 5, 4)
    assert api.png_out_layout(api.png_info(d16)[1], "native", "native") == (2, 2, 60)
    with pytest.raises(ValueError):
        api.png_decode_batch([d8], mode="bgr")
    with pytest.raises(ValueError):
        api.png_decode_batch([d8], depth=12)
