"""The staging rules the tensor, label and colour-label calls share (include/decode_png.h), without a GPU: on files that end
right after IHDR no call reaches the device, so what IHDR and the box decide -- the whole image for no box or an all-zero one,
E_BOX, E_LABEL before E_BOX, the walk's own status otherwise -- must come out of all five entry points alike."""
import ctypes as C
import os
import struct
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_spec_ref as R  # noqa: E402

DUMMY = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced: the calls below never reach the device
GRAY, NEAREST, PACK = 2, 2, 0
U8, U16, I32, I64 = range(4)
E_BOX, E_LABEL = 14, 15
SENTINEL = 0xABCD


class Box(C.Structure):  # include/decode_png.h: debig_png_box
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


class Info(C.Structure):  # include/decode_png.h: debig_png_info
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_uint8), ("color_type", C.c_uint8),
                ("interlace", C.c_uint8), ("has_trns", C.c_uint8), ("reserved", C.c_uint32)]


class TensorDesc(C.Structure):  # include/decode_png.h: debig_png_tensor_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("out_format", C.c_uint32), ("out_layout", C.c_uint32),
                ("dtype", C.c_uint32), ("resize_flags", C.c_uint32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


class AlphaDesc(C.Structure):  # include/decode_png.h: debig_png_alpha_desc
    _fields_ = [("mode", C.c_uint32), ("background", C.c_uint16 * 4), ("reserved", C.c_uint32)]


class FilterDesc(C.Structure):  # include/decode_png.h: debig_png_filter_desc
    _fields_ = [("filter", C.c_uint32), ("reserved", C.c_uint32)]


class LabelDesc(C.Structure):  # include/decode_png.h: debig_png_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("reserved", C.c_uint32),
                ("lut", C.POINTER(C.c_int32))]


class ColorLabelDesc(C.Structure):  # include/decode_png.h: debig_png_color_label_desc
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("dtype", C.c_uint32), ("mode", C.c_uint32), ("missing", C.c_int32),
                ("n_maps", C.c_uint32), ("maps", C.c_void_p), ("reserved", C.c_uint32), ("reserved2", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    from debigulator_amd import _native as N

    if not os.path.exists(N.LIB_PATH):
        from debigulator_amd.build import build

        build()
    L = C.CDLL(N.LIB_PATH)
    for name, extra in (("tensor", 1), ("tensor_alpha", 2), ("tensor_filter", 3), ("labels", 1)):
        f = getattr(L, "debig_png_decode_batch_" + name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * extra
    L.debig_png_decode_batch_color_labels.restype = C.c_int
    L.debig_png_decode_batch_color_labels.argtypes = [C.c_void_p] * 7 + [C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def _ihdr_only(w, h, depth=8, ct=0):
    """the signature and a valid IHDR, nothing behind them"""
    body = b"IHDR" + struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, 0)
    return bytes(R.SIG) + struct.pack(">I", 13) + body + struct.pack(">I", zlib.crc32(body))


def _tensor_desc():
    d = TensorDesc(out_w=8, out_h=6, out_format=GRAY, dtype=1, resize_flags=1)
    for k in range(4):
        d.scale[k] = 1.0
    return d


def _calls(lib, label_dtype=I32, color_dtype=I32):
    """name -> f(ins, sizes, boxes, status, infos, n) of the five entry points"""
    td, ad, fd = _tensor_desc(), AlphaDesc(mode=0), FilterDesc(filter=NEAREST)
    ld, cd = LabelDesc(out_w=8, out_h=6, dtype=label_dtype), ColorLabelDesc(out_w=8, out_h=6, dtype=color_dtype, mode=PACK)
    return {
        "tensor": lambda i, s, b, st, inf, n: lib.debig_png_decode_batch_tensor(i, s, DUMMY, b, st, inf, n, 0, C.byref(td)),
        "tensor_alpha": lambda i, s, b, st, inf, n: lib.debig_png_decode_batch_tensor_alpha(i, s, DUMMY, b, st, inf, n, 0, C.byref(td),
                                                                                            C.byref(ad)),
        "tensor_filter": lambda i, s, b, st, inf, n: lib.debig_png_decode_batch_tensor_filter(i, s, DUMMY, b, st, inf, n, 0,
                                                                                              C.byref(td), C.byref(ad), C.byref(fd)),
        "labels": lambda i, s, b, st, inf, n: lib.debig_png_decode_batch_labels(i, s, DUMMY, b, st, inf, n, 0, C.byref(ld)),
        "color_labels": lambda i, s, b, st, inf, n: lib.debig_png_decode_batch_color_labels(i, s, DUMMY, b, st, inf, None, n, 0,
                                                                                            C.byref(cd)),
    }


def _run(call, files, boxes):
    n = len(files)
    bufs = [C.create_string_buffer(f, len(f)) for f in files]
    ins = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * n)(*[len(f) for f in files])
    st = (C.c_uint32 * n)(*[SENTINEL] * n)
    infos = (Info * n)()
    C.memset(infos, 0xAB, C.sizeof(infos))
    bx = (Box * n)(*[Box(*b) if b else Box(0, 0, 0, 0) for b in boxes]) if boxes is not None else None
    rc = call(ins, sizes, bx, st, infos, n)
    return rc, list(st), [(i.width, i.height, i.bit_depth, i.color_type, i.interlace, i.has_trns) for i in infos]


def test_the_box_rule_is_one_rule_in_all_five_calls(lib):
    big, one, bad_sig = _ihdr_only(45, 70), _ihdr_only(1, 1), b"\x88" + _ihdr_only(45, 70)[1:]
    #        no box, all zero: the whole image; past the right edge; past the bottom edge; zero width; exactly the whole image
    files = [big, big, big, big, big, big, big, one, one, one, one, bad_sig, bad_sig]
    boxes = [None, (0, 0, 0, 0), (1, 0, 45, 70), (0, 1, 45, 70), (3, 3, 0, 2), (0, 0, 45, 70), (44, 69, 1, 1),
             None, (0, 0, 1, 1), (1, 0, 1, 1), (0, 0, 1, 2), None, (0, 0, 46, 70)]
    C_, B, S = R.E_CHUNK, E_BOX, R.E_SIGNATURE
    want = [C_, C_, B, B, B, C_, C_, C_, C_, B, B, S, S]
    info = {big: (45, 70, 8, 0, 0, 0), one: (1, 1, 8, 0, 0, 0), bad_sig: (0, 0, 0, 0, 0, 0)}
    got = {name: _run(call, files, boxes) for name, call in _calls(lib).items()}
    assert got["tensor"] == (0, want, [info[f] for f in files])
    for name, res in got.items():
        assert res == got["tensor"], name
    # no boxes at all: the whole image everywhere
    for name, call in _calls(lib).items():
        assert _run(call, [big, one, bad_sig], None) == (0, [C_, C_, S], [info[big], info[one], info[bad_sig]]), name


def test_label_outranks_box_in_both_label_calls(lib):
    g16 = _ihdr_only(45, 70, 16)
    files, boxes = [g16, g16, g16], [(1, 0, 45, 70), (3, 3, 0, 2), None]
    want = (0, [E_LABEL] * 3, [(45, 70, 16, 0, 0, 0)] * 3)
    assert _run(_calls(lib, label_dtype=U8)["labels"], files, boxes) == want
    for dtype in (I32, I64):
        assert _run(_calls(lib, color_dtype=dtype)["color_labels"], files, boxes) == want
    # where 16 bits are no label error the box is judged: the label call with a wide dtype, and the tensor call
    for name in ("labels", "tensor"):
        assert _run(_calls(lib, label_dtype=U16)[name], files, boxes)[1] == [E_BOX, E_BOX, R.E_CHUNK], name
