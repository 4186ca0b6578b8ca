"""debig_png_decode_batch on the MI355X (include/decode_png.h): every valid format against the reference decoder of
tests/png_spec_ref.py, the resource PNGs against PIL and decode_png, the tuned and the general kernel byte for byte,
every error status, and the size extremes."""
import glob
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "resources", "*.png")))


@pytest.fixture(scope="module")
def api(gpu_device):
    from debigulator_amd import api as A

    return A


def _format_file(rng, ct, depth, il, trns, w=45, h=70, mode="default", filters=None):
    pal = None
    t = None
    if ct == 3:
        n_pal = int(rng.integers(2, (1 << depth) + 1))
        pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(n_pal)]
        s = R.random_image(rng, w, h, ct, depth, n_pal)
        if trns:
            t = bytes(rng.integers(0, 256, size=n_pal - 1, dtype=np.uint8))
    else:
        s = R.random_image(rng, w, h, ct, depth)
        if trns and ct in (0, 2):
            s = s % 3 if depth != 16 else (s % 3) * 257
            t = np.asarray(s[0, 0][: 3 if ct == 2 else 1], dtype=">u2").tobytes()
    return R.encode(s, ct, depth, il, trns=t, palette=pal, mode=mode, filters=filters, idat_split=[7] if il else None)


def _all_formats():
    rng = np.random.default_rng(2024)
    files = []
    for ct, depths in R.DEPTHS.items():
        for depth in depths:
            for il in (0, 1):
                for trns in ((0, 1) if ct in (0, 2, 3) else (0,)):
                    mode = ("stored", "fixed", "default")[(ct + depth + il) % 3]
                    files.append(((ct, depth, il, trns), _format_file(rng, ct, depth, il, trns, mode=mode)))
    return files


def _check_against_reference(out, files):
    for (key, data), (st, px, inf) in zip(files, out):
        est, epx, einf = R.decode(data)
        assert est == R.OK
        assert st == 0, (key, st)
        assert inf == einf, key
        assert np.array_equal(px, epx), (key, np.argwhere(px != epx)[:4])


def test_every_format_matches_reference(api):
    files = _all_formats()
    _check_against_reference(api.png_decode_batch([d for _, d in files]), files)


def test_every_format_one_file_at_a_time(api):
    files = _all_formats()
    for f in files:
        _check_against_reference(api.png_decode_batch([f[1]]), [f])


def test_resource_files_match_pil_and_decode_png(api, monkeypatch):
    PIL = pytest.importorskip("PIL.Image")
    import io

    datas = [open(p, "rb").read() for p in RESOURCES]
    assert len(datas) == 15
    out = api.png_decode_batch(datas)
    monkeypatch.setenv("DEBIG_STRICT", "1")
    for p, data, (st, px, inf) in zip(RESOURCES, datas, out):
        assert st == 0, p
        assert np.array_equal(px, np.asarray(PIL.open(io.BytesIO(data)).convert("RGBA"))), p
        good, flat = api.decode_png(data)
        assert good == 1, p
        assert np.array_equal(px.reshape(-1), flat), p


def test_resource_files_match_reference_decoder_without_pil(api):
    datas = [open(p, "rb").read() for p in RESOURCES]
    for p, data, (st, px, _) in zip(RESOURCES, datas, api.png_decode_batch(datas, force_general=True)):
        est, epx, _ = R.decode(data)
        assert st == est == 0, p
        assert np.array_equal(px, epx), p


def test_tuned_and_general_kernels_agree(api):
    """8-bit RGB / RGBA, non-interlaced: the tuned de-filter and the general kernel, byte for byte -- including images
    whose IDAT streams are long enough to take the chunk-task inflate"""
    rng = np.random.default_rng(77)
    files = []
    for k, (w, h) in enumerate([(1, 1), (5, 3), (64, 65), (333, 129), (1024, 700), (1500, 1100)]):
        for ct in (2, 6):
            s = R.random_image(rng, w, h, ct, 8)
            if w * h > 100000:  # smooth content: long IDAT streams of short matches
                y, x = np.mgrid[0:h, 0:w]
                s = ((x[:, :, None] * (k + 1) + y[:, :, None] * 3 + np.arange(R.CHANNELS[ct])) // 5 % 256).astype(np.uint8)
                s = (s + rng.integers(0, 3, size=s.shape)).astype(np.uint8)
            files.append(R.encode(s, ct, 8, filters=lambda p, y: y % 5))
    # every stream of a batch long: the chunk-task inflate (include/debig_hip.h: DEBIG_WAVES_CHUNKED)
    large = [R.encode(R.random_image(rng, 700, 500, ct, 8), ct, 8, filters=lambda p, y: (0, 2)[y % 2]) for ct in (6, 2, 6)]
    for batch in (files, large):
        a = api.png_decode_batch(batch)
        b = api.png_decode_batch(batch, force_general=True)
        for data, (sa, pa, inf), (sb, pb, _) in zip(batch, a, b):
            assert sa == sb == 0
            assert np.array_equal(pa, pb)
            if inf["width"] * inf["height"] <= 200_000:
                assert np.array_equal(pa, R.decode(data)[1])


def _error_files():
    rng = np.random.default_rng(5)
    s = R.random_image(rng, 20, 11, 6, 8)
    raw = R.scanlines(s, 6, 8)
    z = zlib.compress(raw)
    good = R.encode(s, 6, 8, zdata=z)
    crc = bytearray(good)
    crc[50] ^= 0x10  # inside IDAT: the stored CRC no longer matches
    cases = [("crc", bytes(crc), R.E_CRC),
             ("adler wrong", R.encode(s, 6, 8, zdata=z[:-4] + bytes(4)), R.E_ADLER),
             ("adler missing", R.encode(s, 6, 8, zdata=z[:-4]), R.E_ADLER),
             ("short data", R.encode(s, 6, 8, zdata=zlib.compress(raw[:-5])), R.E_DATA_SHORT),
             ("long data", R.encode(s, 6, 8, zdata=zlib.compress(raw + bytes(9))), R.E_DATA_LONG),
             ("inflate", R.encode(s, 6, 8, zdata=z[:2] + bytes([0x01, 5, 0, 0, 0]) + z[7:]), R.E_INFLATE),  # stored LEN != ~NLEN
             ("filter 5", R.encode(s, 6, 8, filters=lambda p, y: 5 if y == 7 else 1), R.E_FILTER),
             ("filter 5 interlaced", R.encode(R.random_image(rng, 9, 9, 0, 4), 0, 4, 1, filters=lambda p, y: 5 if p == 6 else 2), R.E_FILTER),
             ("palette index", R.encode(np.full((5, 6, 1), 3, np.uint8), 3, 8, palette=[(1, 2, 3)] * 3), R.E_PALETTE),
             ("palette index 2-bit", R.encode(np.full((5, 6, 1), 3, np.uint8), 3, 2, 1, palette=[(1, 2, 3)] * 2), R.E_PALETTE)]
    fl = 0x20 | ((31 - ((0x78 << 8) | 0x20) % 31) % 31)
    cases.append(("fdict", R.encode(s, 6, 8, zdata=bytes([0x78, fl]) + b"\0\0\0\1" + z[2:]), R.E_ZLIB))
    for name, data, st in cases:
        assert R.decode(data)[0] == st, name
    return cases


def test_every_error_status_beside_good_files(api):
    cases = _error_files()
    files = _all_formats()[::3]
    batch, expect = [], []
    for k, (name, data, st) in enumerate(cases):
        batch.append(data)
        expect.append((name, st))
        batch.append(files[k % len(files)][1])
        expect.append(("good", 0))
    out = api.png_decode_batch(batch)
    for data, (name, st), (got, px, _) in zip(batch, expect, out):
        assert got == st, (name, got)
        if st == 0:
            assert np.array_equal(px, R.decode(data)[1])
    # the same files one by one, and through the general kernel
    for name, data, st in cases:
        assert api.png_decode_batch([data])[0][0] == st, name
        assert api.png_decode_batch([data], force_general=True)[0][0] == st, name


def test_output_cap_too_small(api):
    import ctypes as C

    from debigulator_amd import _native as N

    rng = np.random.default_rng(8)
    datas = [R.encode(R.random_image(rng, 13, 9, 2, 16), 2, 16), R.encode(R.random_image(rng, 13, 9, 6, 8), 6, 8)]
    L = api._png_spec_lib()
    outs = [np.zeros(4 * 13 * 9, np.uint8) for _ in datas]
    ins = [np.frombuffer(d, np.uint8) for d in datas]
    st = (C.c_uint32 * 2)()
    rc = L.debig_png_decode_batch((C.c_void_p * 2)(*[a.ctypes.data for a in ins]), (C.c_uint64 * 2)(*[len(d) for d in datas]),
                                  (C.c_void_p * 2)(*[o.ctypes.data for o in outs]), (C.c_uint64 * 2)(4 * 13 * 9 - 1, 4 * 13 * 9),
                                  st, None, 2, 0)
    N.check(rc, "debig_png_decode_batch")
    assert list(st) == [R.E_OUTPUT, 0]
    assert np.array_equal(outs[1].reshape(9, 13, 4), R.decode(datas[1])[1])


def test_size_extremes(api):
    rng = np.random.default_rng(9)
    one = R.encode(np.array([[[7, 8, 9, 10]]], np.uint8), 6, 8)
    one_il = R.encode(np.array([[[40000]]], np.uint16), 0, 16, 1, trns=b"\x9c\x40")
    wide = R.encode(R.random_image(rng, 16384, 3, 0, 1), 0, 1, filters=lambda p, y: (1, 4, 3)[y])
    big16 = R.encode(R.random_image(rng, 8192, 64, 6, 16), 6, 16, filters=lambda p, y: (0, 1, 2)[y % 3])
    files = [one, one_il, wide, big16]
    out = api.png_decode_batch(files)
    for data, (st, px, _) in zip(files, out):
        assert st == 0
        assert np.array_equal(px, R.decode(data)[1])
    assert out[1][1].tolist() == [[[156, 156, 156, 0]]]
