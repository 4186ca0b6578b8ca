"""The spec-complete PNG path without a GPU: the reference decoder of tests/png_spec_ref.py against PIL and against
itself (metamorphic checks), and the statuses debig_png_decode_batch decides on the host."""
import ctypes as C
import glob
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "resources", "*.png")))


def _pil_rgba(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


# ------------------------------------------------------------------------------------------------ vs PIL
@pytest.mark.parametrize("mode", ["L", "LA", "RGB", "RGBA", "P1", "P2", "P4", "P8", "1", "I;16"])
def test_reference_decoder_on_pil_files(mode):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(len(mode))
    w, h = 53, 31
    kw = {}
    if mode in ("L", "LA", "RGB", "RGBA"):
        ch = len(mode)
        im = Image.fromarray(rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8).squeeze(), mode)
    elif mode == "1":
        im = Image.fromarray(rng.integers(0, 2, size=(h, w), dtype=np.uint8) * 255, "L").convert("1")
    elif mode == "I;16":
        im = Image.fromarray(rng.integers(0, 65536, size=(h, w), dtype=np.uint16))
        assert im.mode == "I;16"
    else:
        bits = int(mode[1])
        n = 1 << bits
        im = Image.fromarray(rng.integers(0, n, size=(h, w), dtype=np.uint8), "P")
        im.putpalette(list(rng.integers(0, 256, size=3 * n, dtype=np.uint8)))
        kw = dict(bits=bits, transparency=bytes(rng.integers(0, 256, size=n // 2 + 1, dtype=np.uint8)))
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    data = buf.getvalue()
    st, px, inf = R.decode(data)
    assert st == R.OK
    if mode == "I;16":  # PIL's RGBA of a 16-bit grey image clips instead of reducing: compare the raw samples
        assert inf["bit_depth"] == 16
        assert np.array_equal(px[:, :, 0], (np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8))
        return
    assert np.array_equal(px, _pil_rgba(data))


@pytest.mark.parametrize("ct,depth", [(0, 16), (2, 16), (4, 16), (6, 16), (0, 8), (2, 8), (6, 8), (3, 4), (0, 2)])
def test_reference_decoder_on_own_interlaced_and_16bit_files(ct, depth):
    """the helper's encoder (Adam7, 16-bit, mixed filters) against PIL: raw samples where PIL exposes them"""
    pytest.importorskip("PIL")
    from PIL import Image

    rng = np.random.default_rng(ct * 31 + depth)
    pal = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(16)] if ct == 3 else None
    s = R.random_image(rng, 27, 19, ct, depth, 16 if ct == 3 else None)
    for il in (0, 1):
        data = R.encode(s, ct, depth, il, palette=pal, mode=("stored", "fixed", "default")[il + ct % 2])
        st, px, _ = R.decode(data)
        assert st == R.OK
        im = Image.open(io.BytesIO(data))
        if depth == 16 and ct == 0:
            raw = np.asarray(im).astype(np.uint32)
            assert np.array_equal(px[:, :, 0], (raw >> 8).astype(np.uint8))
        elif depth == 16:
            # PIL reduces 16-bit colour to 8 bits on load the same way (high byte)
            assert np.array_equal(px, _pil_rgba(data))
        else:
            assert np.array_equal(px, _pil_rgba(data))


@pytest.mark.parametrize("path", RESOURCES, ids=[os.path.basename(p) for p in RESOURCES])
def test_reference_decoder_on_resource_files(path):
    pytest.importorskip("PIL")
    data = open(path, "rb").read()
    st, px, _ = R.decode(data)
    assert st == R.OK
    assert np.array_equal(px, _pil_rgba(data))


def test_resource_files_present():
    assert len(RESOURCES) == 15


# ------------------------------------------------------------------------------------------------ metamorphic
@pytest.mark.parametrize("ct,depth", [(0, 1), (0, 4), (0, 16), (2, 8), (2, 16), (3, 2), (4, 16), (6, 8), (6, 16)])
def test_interlaced_and_plain_encodings_decode_equally(ct, depth):
    rng = np.random.default_rng(depth + 10 * ct)
    for w, h in ((1, 1), (3, 7), (9, 4), (40, 33)):
        pal = [(i, 255 - i, i // 2) for i in range(1 << depth)] if ct == 3 else None
        s = R.random_image(rng, w, h, ct, depth)
        a = R.decode(R.encode(s, ct, depth, 0, palette=pal, mode="fixed"))
        b = R.decode(R.encode(s, ct, depth, 1, palette=pal, idat_split=[1, 5]))
        assert a[0] == b[0] == R.OK
        assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("ct", [0, 2, 4, 6])
def test_16bit_with_8bit_high_bytes_decodes_like_8bit(ct):
    rng = np.random.default_rng(ct)
    s8 = R.random_image(rng, 21, 17, ct, 8)
    low = rng.integers(0, 256, size=s8.shape, dtype=np.uint16)
    s16 = (s8.astype(np.uint16) << 8) | low
    for il in (0, 1):
        a = R.decode(R.encode(s8, ct, 8, il))
        b = R.decode(R.encode(s16, ct, 16, il))
        assert a[0] == b[0] == R.OK
        assert np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ host rules
class PngInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8), ("color_type", C.c_uint8),
                ("interlace", C.c_uint8), ("has_trns", C.c_uint8), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    L.debig_png_info_get.restype = C.c_uint32
    L.debig_png_info_get.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(PngInfo)]
    L.debig_png_decode_batch.restype = C.c_int
    L.debig_png_decode_batch.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32]
    return L


def _host_status(L, datas, caps=None):
    """debig_png_decode_batch on files that all fail on the host: no device work happens"""
    n = len(datas)
    bufs = [C.create_string_buffer(bytes(d), max(len(d), 1)) for d in datas]
    outs = [C.create_string_buffer(64) for _ in datas]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(d) for d in datas])
    optr = (C.c_void_p * n)(*[C.addressof(o) for o in outs])
    cap = (C.c_uint64 * n)(*(caps or [64] * n))
    st = (C.c_uint32 * n)()
    infos = (PngInfo * n)()
    assert L.debig_png_decode_batch(ins, sizes, optr, cap, st, infos, n, 0) == 0
    return list(st)


def _body(data, typ):
    """(offset of the chunk's length field, body) of the first chunk of this type"""
    pos = 8
    while pos < len(data):
        ln = struct.unpack(">I", data[pos: pos + 4])[0]
        if data[pos + 4: pos + 8] == typ:
            return pos, data[pos + 8: pos + 8 + ln]
        pos += 12 + ln
    raise KeyError(typ)


def _ihdr(w, h, d, ct, comp=0, filt=0, il=0):
    return struct.pack(">IIBBBBB", w, h, d, ct, comp, filt, il)


def _bad_files():
    rng = np.random.default_rng(3)
    s = R.random_image(rng, 3, 2, 2, 8)
    good = R.encode(s, 2, 8)
    pal = [(1, 2, 3), (4, 5, 6)]
    sp = np.zeros((2, 3, 1), dtype=np.uint8)
    cases = []
    cases.append(("signature", b"\x89PNG\r\n\x1a\x0b" + good[8:], R.E_SIGNATURE))
    cases.append(("short signature", good[:6], R.E_SIGNATURE))
    cases.append(("IHDR not first", R.SIG + R.chunk(b"tEXt", b"a\0b") + good[8:], R.E_CHUNK))
    cases.append(("two IHDR", good[:33] + good[8:33] + good[33:], R.E_CHUNK))
    cases.append(("IHDR length", R.encode(s, 2, 8, ihdr=_ihdr(3, 2, 8, 2) + b"\0"), R.E_IHDR))
    for d, ct in ((8, 1), (16, 3), (4, 2), (2, 4), (1, 6), (3, 0), (32, 0)):
        cases.append(("pair %d/%d" % (ct, d), R.encode(s, 2, 8, ihdr=_ihdr(3, 2, d, ct)), R.E_IHDR))
    cases.append(("compression", R.encode(s, 2, 8, ihdr=_ihdr(3, 2, 8, 2, comp=1)), R.E_IHDR))
    cases.append(("filter method", R.encode(s, 2, 8, ihdr=_ihdr(3, 2, 8, 2, filt=1)), R.E_IHDR))
    cases.append(("interlace 2", R.encode(s, 2, 8, ihdr=_ihdr(3, 2, 8, 2, il=2)), R.E_IHDR))
    cases.append(("width 0", R.encode(s, 2, 8, ihdr=_ihdr(0, 2, 8, 2)), R.E_IHDR))
    cases.append(("height 2^31", R.encode(s, 2, 8, ihdr=_ihdr(3, 1 << 31, 8, 2)), R.E_IHDR))
    cases.append(("no PLTE", R.encode(sp, 3, 8), R.E_CHUNK))
    cases.append(("PLTE on grey", R.encode(sp, 0, 8, palette=pal), R.E_CHUNK))
    cases.append(("PLTE on grey+alpha", R.encode(np.zeros((2, 3, 2), np.uint8), 4, 8, palette=pal), R.E_CHUNK))
    cases.append(("PLTE length", R.encode(sp, 3, 8, extra_before_idat=[(b"PLTE", b"\1\2\3\4")]), R.E_PALETTE))
    cases.append(("PLTE 257 entries", R.encode(sp, 3, 8, extra_before_idat=[(b"PLTE", bytes(771))]), R.E_PALETTE))
    cases.append(("two PLTE", R.encode(sp, 3, 8, palette=pal, extra_before_idat=[(b"PLTE", bytes(6))]), R.E_CHUNK))
    cases.append(("unknown critical", R.encode(s, 2, 8, extra_before_idat=[(b"ABCD", b"x")]), R.E_CHUNK))
    pos, _ = _body(good, b"IDAT")
    idat = good[pos: pos + 12 + struct.unpack(">I", good[pos: pos + 4])[0]]
    cases.append(("IDAT not consecutive", good[:pos] + idat + R.chunk(b"tEXt", b"k\0v") + idat + good[pos + len(idat):], R.E_CHUNK))
    cases.append(("no IDAT", good[:pos] + good[pos + len(idat):], R.E_CHUNK))
    cases.append(("no IEND", good[:-12], R.E_CHUNK))
    cases.append(("truncated chunk", good[:-14], R.E_CHUNK))
    cases.append(("truncated header", good[:20], R.E_CHUNK))
    z = R.zlib_stream(R.scanlines(s, 2, 8))
    cases.append(("zlib CM", R.encode(s, 2, 8, zdata=bytes([0x77]) + z[1:]), R.E_ZLIB))
    cases.append(("zlib CINFO", R.encode(s, 2, 8, zdata=bytes([0x88, (31 - (0x88 << 8) % 31) % 31]) + z[2:]), R.E_ZLIB))
    cases.append(("zlib FCHECK", R.encode(s, 2, 8, zdata=bytes([z[0], z[1] ^ 1]) + z[2:]), R.E_ZLIB))
    fl = 0x20 | ((31 - ((0x78 << 8) | 0x20) % 31) % 31)
    cases.append(("zlib FDICT", R.encode(s, 2, 8, zdata=bytes([0x78, fl]) + b"\0\0\0\0" + z[2:]), R.E_ZLIB))
    cases.append(("zlib 1 byte", R.encode(s, 2, 8, zdata=z[:1]), R.E_ZLIB))
    return cases


def test_host_statuses(lib):
    cases = _bad_files()
    for name, data, st in cases:
        assert R.decode(data)[0] == st, name  # the reference decoder agrees
    got = _host_status(lib, [d for _, d, _ in cases])
    assert got == [st for _, _, st in cases], [(c[0], g) for c, g in zip(cases, got) if g != c[2]]


def test_output_too_small_is_decided_on_the_host(lib):
    rng = np.random.default_rng(1)
    data = R.encode(R.random_image(rng, 5, 4, 6, 8), 6, 8)
    assert _host_status(lib, [data], caps=[4 * 5 * 4 - 1]) == [R.E_OUTPUT]
    assert R.decode(data, out_cap=79)[0] == R.E_OUTPUT


def test_info_get(lib):
    rng = np.random.default_rng(2)
    cases = [(R.encode(R.random_image(rng, 7, 5, 0, 16), 0, 16, 1, trns=b"\0\7"), (7, 5, 16, 0, 1, 1)),
             (R.encode(R.random_image(rng, 9, 3, 3, 2, 3), 3, 2, palette=[(1, 1, 1)] * 3, trns=b"\0"), (9, 3, 2, 3, 0, 1)),
             (R.encode(R.random_image(rng, 2, 2, 4, 8), 4, 8, trns=b"\0\0"), (2, 2, 8, 4, 0, 0)),  # tRNS on type 4: ignored
             (R.encode(R.random_image(rng, 2, 2, 2, 8), 2, 8, trns=b"\0\0"), (2, 2, 8, 2, 0, 0))]  # wrong length: ignored
    for data, exp in cases:
        inf = PngInfo()
        assert lib.debig_png_info_get(data, len(data), C.byref(inf)) == 0
        got = (inf.width, inf.height, inf.bit_depth, inf.color_type, inf.interlace, inf.has_trns)
        assert got == exp
        st, ref = R.info(data)
        assert st == 0 and tuple(ref[k] for k in ("width", "height", "bit_depth", "color_type", "interlace", "has_trns")) == exp
    inf = PngInfo()
    assert lib.debig_png_info_get(b"GIF89a", 6, C.byref(inf)) == R.E_SIGNATURE
    bad = R.encode(np.zeros((1, 1, 1), np.uint8), 0, 8, ihdr=_ihdr(1, 1, 16, 3))
    assert lib.debig_png_info_get(bad, len(bad), C.byref(inf)) == R.E_IHDR


def test_reference_decoder_device_statuses():
    """the statuses the GPU decides, as the reference decoder sees them (the GPU tests check the library)"""
    rng = np.random.default_rng(9)
    s = R.random_image(rng, 6, 5, 6, 8)
    raw = R.scanlines(s, 6, 8)
    z = zlib.compress(raw)
    good = R.encode(s, 6, 8, zdata=z)
    assert R.decode(good)[0] == R.OK
    bad_crc = bytearray(good)
    bad_crc[-1] ^= 1  # IEND's CRC
    assert R.decode(bytes(bad_crc))[0] == R.E_CRC
    assert R.decode(R.encode(s, 6, 8, zdata=z[:-4] + bytes(4)))[0] == R.E_ADLER
    assert R.decode(R.encode(s, 6, 8, zdata=z[:-4]))[0] == R.E_ADLER
    assert R.decode(R.encode(s, 6, 8, zdata=zlib.compress(raw[:-3])))[0] == R.E_DATA_SHORT
    assert R.decode(R.encode(s, 6, 8, zdata=zlib.compress(raw + b"\0")))[0] == R.E_DATA_LONG
    assert R.decode(R.encode(s, 6, 8, zdata=z[:2] + b"\xff" * 8 + z[10:]))[0] == R.E_INFLATE
    assert R.decode(R.encode(s, 6, 8, filters=lambda p, y: 5 if y == 3 else 0))[0] == R.E_FILTER
    sp = np.full((2, 2, 1), 2, np.uint8)
    assert R.decode(R.encode(sp, 3, 8, palette=[(0, 0, 0), (1, 1, 1)]))[0] == R.E_PALETTE
